"""The open-side authentication matrix (tests/open_matrix.py) through the AES-GCM batch API on the device (used by
tests/test_gpu_open_matrix.py).

`run` opens one list of cases in one launch, with `result` pre-filled with a sentinel and the output buffer with 0xA5, and
compares with the CPU oracle's `open` of the same claimed fields and presented bytes: the verdict of every record, the
claimed-length output bytes of every record (damaged ones included: decrypt-then-verify) and every other byte of the output
buffer, which must be unchanged.

Run as a script (`python open_matrix_case.py LANES KEY_LEN`) it prints, for whichever libptls_hip.so PTLS_HIP_LIB names, a
MISMATCHES line with the damaged cases that were accepted and the intact ones that were rejected: the test runs it on the
TEST-ONLY mutant build (hsig-picotls_amd/mutants/libptls_hip_open1.so, batch_kernel.h OPEN_MUTANT) and expects exactly
the cases that mutant must let through.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "hsig-picotls_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import open_matrix as om  # noqa: E402

UINT64_MAX = (1 << 64) - 1
SENTINEL = 0x5A5A5A5A5A5A5A5A  # `result` before the launch: neither a length nor UINT64_MAX
FILL = 0xA5
SPARSE_N = (41, 154)  # GHASH elements of the lanes = 64 shapes: one wave without a Horner step, two pairs of waves


def base(oracle, key_len, L, A, j=0):
    key, iv = oracle.gen_key(900 + j, key_len)
    return key, iv, om.BASE_SEQ, oracle.stream(7100 + j, A), oracle.stream(7200 + j, L)


@functools.lru_cache(maxsize=None)
def batch_cases(oracle, key_len, G):
    """the full matrix at the batch kernel's base shape of G lanes per record, all records under one key"""
    return tuple(om.matrix(base(oracle, key_len, om.aes_len(G), om.AAD_LEN), oracle.seal))


@functools.lru_cache(maxsize=None)
def sparse_cases(oracle, key_len, N):
    """the full matrix at N GHASH elements, every record under a key of its own (and so with a ciphertext of its own)"""
    L = om.aes_len_of_elements(N)
    return tuple(om.matrix(lambda i: base(oracle, key_len, L, om.AAD_LEN, 1 + i), oracle.seal))


@functools.lru_cache(maxsize=None)
def tiny_cases(oracle, key_len):
    """T and the existing L cases of the four tiny shapes, under one key, in one list"""
    out = []
    for s, (L, A) in enumerate(om.TINY_SHAPES):
        key, iv, seq, aad, pt = base(oracle, key_len, L, A)
        out += om.matrix((key, iv, seq + 1000 * s, aad, pt), oracle.seal, kinds="TL", seed=2024 + s)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(oracle, cases):
    return tuple(om.verdicts(cases, oracle.open))


def run(engine, oracle, cases, lanes, wg=0, align=16, in_place=False):
    """one open launch of `cases`.  Returns (results, expected results, output image, expected image)."""
    from hip_helpers import HostBatch
    recs = [(c.key, c.iv, c.seq, c.aad, bytes(om.claimed_len(c))) for c in cases]
    hb = HostBatch(engine, recs, align=align)
    res, _ = hb.open([c.sealed for c in cases], lanes, wg=wg, in_place=in_place, out_fill=FILL, res_fill=SENTINEL)
    assert in_place or hb.batch.lanes == lanes
    want = expected(oracle, tuple(cases))
    want_res = [om.claimed_len(c) if ok else UINT64_MAX for c, (ok, _) in zip(cases, want)]
    img = np.full(len(hb.out_image), FILL, np.uint8)
    for c, (_, pt), off in zip(cases, want, hb.out_offs):
        if in_place:  # the presented bytes, then the record's output over its first claimed-length bytes: the tag stays
            img[off: off + len(c.sealed)] = np.frombuffer(c.sealed, np.uint8)
        if len(pt):
            img[off: off + len(pt)] = np.frombuffer(pt, np.uint8)
    out = hb.out_image
    hb.close()
    return res, want_res, out, img


def report(cases, res, want_res, out, img):
    """(damaged cases accepted, intact cases rejected, records whose result is neither verdict or the wrong length,
    output bytes that differ from the expected image) -- the first three as 'kind:what' strings"""
    def name(c):
        return f"{c.kind}:" + ("-".join(str(x) for x in c.what) if isinstance(c.what, tuple) else str(c.what))
    accepted = [name(c) for c, r in zip(cases, res) if c.kind != "I" and r == om.claimed_len(c)]
    rejected = [name(c) for c, r in zip(cases, res) if c.kind == "I" and r == UINT64_MAX]
    other = [name(c) for c, r, w in zip(cases, res, want_res) if r != w and r not in (UINT64_MAX, om.claimed_len(c))]
    return accepted, rejected, other, int((out != img).sum())


def check(engine, oracle, cases, lanes, **kw):
    res, want_res, out, img = run(engine, oracle, cases, lanes, **kw)
    damaged = sum(1 for c in cases if c.kind != "I")
    assert want_res.count(UINT64_MAX) == damaged and 4 * (len(cases) - damaged) >= len(cases)
    accepted, rejected, other, diff = report(cases, res, want_res, out, img)
    assert (accepted, rejected, other) == ([], [], []), (f"{len(accepted)} damaged records accepted {accepted[:8]}, "
                                                         f"{len(rejected)} intact rejected {rejected[:8]}, "
                                                         f"{len(other)} with neither verdict {other[:8]}")
    assert res == want_res
    assert diff == 0, f"{diff} output bytes differ from the oracle's open / the 0x{FILL:02X} fill, first at " \
                      f"{np.flatnonzero(out != img)[:8].tolist()}"
    return res, out


def main():
    lanes, key_len = int(sys.argv[1]), int(sys.argv[2])
    import torch
    # torch first: its HIP runtime must be the process's one before libptls_hip.so loads (as tests/dealing_case.py)
    assert torch.cuda.is_available()
    import ptls_hip
    from oracle_lib import Oracle
    o = Oracle()
    eng = ptls_hip.Engine(0)
    cases = batch_cases(o, key_len, lanes)
    accepted, rejected, other, diff = report(cases, *run(eng, o, cases, lanes, wg=768))
    eng.close()
    print(f"MISMATCHES accepted={','.join(accepted)} rejected={','.join(rejected)} other={','.join(other)} bytes={diff} "
          f"lib={ptls_hip.LIB_PATH}", flush=True)


if __name__ == "__main__":
    main()
