"""The open-side authentication matrix (tests/open_matrix.py) through the ChaCha20-Poly1305 batch kernel.

Per lanes-per-record G and layout, one launch opens intact records shuffled with records damaged in one field as the opener
sees it: at L = 64 (2 G + 1) + 17, A = 21 (two full trips of G blocks per record, one more block and a 17-byte tail) each
of the 128 tag bits, a bit in every 64-byte ciphertext block and in the first and last byte of the tail, a bit in every AAD
byte, and the six length cases in which the bytes hashed are the base's and only Poly1305's length block differs; at
L = 129 each of the 64 sequence-number bits and a bit in every static-IV and key byte (under key slots of their own), plus
four sequence-number bits at the long shape.  Expected verdicts and bytes: tests/chacha_ref.py, with the keystream computed
once per (key, nonce) and shared by the cases that keep both (chacha_ref.SharedOpen); tests/test_open_matrix_ref.py checks
the lists against that reference alone.  `result` is pre-filled with a sentinel, `out` with 0xA5, and the WHOLE output
buffer is compared: the claimed-length bytes of every record, damaged ones included, are written (decrypt-then-verify) and
nothing else is."""
import functools

import numpy as np
import pytest

import chacha_ref
import open_matrix as om
import ptls_hip
from test_gpu_chacha import GS, U64, Rec, image, run, stream

pytestmark = pytest.mark.gpu

KEY = stream("gpu-chacha-open-matrix-key", 32)
IV = bytes(b | 1 for b in stream("gpu-chacha-open-matrix-iv", 12))
SHORT_LEN = 129
LONG_S_BITS = (0, 31, 32, 63)


@functools.lru_cache(maxsize=None)
def cases_of(g):
    """(cases, expected (accepted, bytes) per case) at lanes-per-record g"""
    L = om.chacha_len(g)
    long_base = (KEY, IV, om.BASE_SEQ, stream("gpu-chacha-open-matrix-aad", om.AAD_LEN), stream("gpu-chacha-open-matrix", L))
    cases = om.matrix(long_base, chacha_ref.seal, kinds="TCAL", chacha=True, extra_intact=2)  # (2 more for the 4 below)
    b, sealed = om.prepare(long_base, chacha_ref.seal)
    extra = [om.apply(b, sealed, ("S", bit)) for bit in LONG_S_BITS]
    for k, c in enumerate(extra):  # spread through the list
        cases.insert((k + 1) * len(cases) // 5, c)
    short_base = (KEY, IV, om.BASE_SEQ ^ (1 << 40), long_base[3], long_base[4][:SHORT_LEN])
    cases += om.matrix(short_base, chacha_ref.seal, kinds="SK", chacha=True, seed=2025)
    want = om.verdicts(cases, om.pt_ok_open(chacha_ref.SharedOpen().open_))
    assert om.false_accepts(cases, [ok for ok, _ in want]) == ([], [])
    return tuple(cases), tuple(want)


@pytest.mark.parametrize("aligned", [False, True], ids=["packed", "aligned16"])
@pytest.mark.parametrize("g", GS)
def test_open_matrix(engine, g, aligned):
    cases, want = cases_of(g)
    slots = {}
    for c in cases:
        slots.setdefault((c.key, c.iv), len(slots))
    assert len(slots) == 1 + 12 + 32
    ks = ptls_hip.KeySet(engine, 32, len(slots), algo=ptls_hip.ALGO_CHACHA20POLY1305)
    ks.set(0, b"".join(k for k, _ in slots), b"".join(iv for _, iv in slots))
    recs = [Rec(slots[(c.key, c.iv)], c.seq, c.aad, bytes(om.claimed_len(c))) for c in cases]
    res, out, base, offs = run(engine, ks, recs, g, aligned, "open", inputs=[c.sealed for c in cases])
    ks.close()
    want_res = [len(pt) if ok else U64 for ok, pt in want]
    wrong = [(c.kind, c.what, r) for c, r, w in zip(cases, res, want_res) if r != w]
    assert not wrong, f"{len(wrong)} of {len(cases)} verdicts differ from the reference, first {wrong[:8]}"
    assert sum(1 for w in want_res if w != U64) * 4 >= len(cases)
    assert np.array_equal(out, image(base, offs, [pt for _, pt in want]))
