"""The full-block stretch's counter-mode window constants (csrc/ctr_window.h) on the device.

Rounds 1-2 of a counter block come from constants that hold for one window of 256 block counters (one value of counter
byte 14) and are stepped in the iteration in which a lane's counter enters the next window.  A window boundary is a data
block c with (c + 2) mod 256 = 0: c = 254, 510, 766.  The lengths 16 k + r, k in 250..262 and 506..518, r in {0, 1, 15},
put the boundary before, inside and after the last stretch iteration and in the generic tail, for every lane phase; the AAD
lengths (0, 1, 1, 1, 2, 2, 4 AAD blocks) shift the lanes' first counters.  All records of a case share one key, so records
of different lengths and AAD lengths share wave tasks: the lanes of one wave cross windows in different iterations and the
stretch ends at the shortest lane.  Reference: the CPU oracle; seal must equal it byte for byte on every record, open must
round-trip, and a tampered tag must fail with the plaintext still written."""
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from hip_helpers import HostBatch  # noqa: E402

UINT64_MAX = (1 << 64) - 1
AADS = (0, 5, 13, 16, 17, 32, 49)
KS = tuple(range(250, 263)) + tuple(range(506, 519))
RS = (0, 1, 15)


def _extra_ks(lanes):
    """lanes 16 and 32 step 2 G blocks per iteration: boundaries of the iterations after block 254"""
    if lanes < 16:
        return ()
    return tuple(254 + 2 * lanes * j + d for j in (1, 2) for d in range(-3, 4))


@functools.lru_cache(maxsize=None)
def _case(o, key_len, extra):
    """(records, expected seals) of one key size: about 300 records of at most 8.4 KiB, computed once and shared
    (o: the session's oracle fixture)"""
    key, iv = o.gen_key(4000 + key_len, key_len)
    recs = []
    for j, (k, r) in enumerate(itertools.product(KS + extra, RS)):
        for i in range(4 if k in KS else 2):
            A = AADS[(j + 2 * i) % len(AADS)]
            n = len(recs)
            recs.append((key, iv, 70_000 + n, o.stream(8000 + n, A), o.stream(9000 + n, 16 * k + r)))
    return tuple(recs), tuple(o.seal(*rec) for rec in recs)


def _check(engine, recs, expect, lanes, wg, align):
    recs = list(recs)
    hb = HostBatch(engine, recs, align=align)
    outs = hb.seal(lanes, wg=wg)
    assert hb.batch.lanes == lanes
    assert len(outs) == len(recs)
    bad = [j for j, (o, e) in enumerate(zip(outs, expect)) if o != e]
    assert not bad, f"{len(bad)} of {len(recs)} records differ from the oracle, first {bad[:8]}"
    res, pts = hb.open(outs, lanes, wg=wg)
    assert res == [len(r[4]) for r in recs]
    assert pts == [r[4] for r in recs]
    # one tampered tag: the failure code, with the plaintext still written (decrypt-then-verify)
    t = len(recs) // 2
    tampered = list(outs)
    b = bytearray(tampered[t])
    b[-3] ^= 0x40
    tampered[t] = bytes(b)
    res, pts = hb.open(tampered, lanes, wg=wg)
    assert res == [UINT64_MAX if j == t else len(r[4]) for j, r in enumerate(recs)]
    assert pts == [r[4] for r in recs]
    hb.close()


@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16, 32])
def test_window_boundaries(engine, oracle, lanes, key_len):
    recs, expect = _case(oracle, key_len, _extra_ks(lanes))
    _check(engine, recs, expect, lanes, 768, 16)


@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("lanes", [4, 32])
def test_window_boundaries_512_threads(engine, oracle, lanes, key_len):
    recs, expect = _case(oracle, key_len, _extra_ks(lanes))
    _check(engine, recs, expect, lanes, 512, 16)


@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("align", [128, 1])
@pytest.mark.parametrize("lanes", [4, 8])
def test_window_boundaries_layouts(engine, oracle, lanes, align, key_len):
    """align 128: every record starts a 128-byte line (the plain loop; 16 above is the deferred-store copy of the loop);
    align 1: the unaligned instantiation"""
    recs, expect = _case(oracle, key_len, _extra_ks(lanes))
    _check(engine, recs, expect, lanes, 768, align)


@functools.lru_cache(maxsize=None)
def _out_of_step(o, key_len):
    rng = np.random.default_rng(77 + key_len)
    key, iv = o.gen_key(4100 + key_len, key_len)
    recs = []
    for n in range(300):
        L = int(rng.integers(3900, 8400))
        A = AADS[int(rng.integers(0, len(AADS)))]
        recs.append((key, iv, 90_000 + n, o.stream(8500 + n, A), o.stream(9500 + n, L)))
    return tuple(recs), tuple(o.seal(*rec) for rec in recs)


@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("lanes", [4, 16])
def test_lanes_out_of_step(engine, oracle, lanes, key_len):
    """records of random lengths (3.9 .. 8.4 KiB, any remainder) and AAD lengths under one key: the records of a wave
    task start their stretch at different counters and the stretch ends at the shortest one, anywhere in a window"""
    recs, expect = _out_of_step(oracle, key_len)
    _check(engine, recs, expect, lanes, 768, 16)
