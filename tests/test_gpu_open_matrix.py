"""The open-side authentication matrix (tests/open_matrix.py) through every AES-GCM kernel path of the batch API.

An open kernel that accepts what it must reject passes every seal-parity and round-trip test.  Here every record of a
launch is either intact or damaged in ONE field as the opener sees it: each tag bit, a bit in every ciphertext block and
every AAD byte, each sequence-number bit, a bit in every static-IV and key byte, and the six length cases in which the
bytes hashed are the base's and only GHASH's length block differs.  Damaged and intact records are shuffled together, so
they share wave tasks.  `result` is pre-filled with a sentinel and `out` with 0xA5; the CPU oracle's `open` of the same
claimed fields and presented bytes gives the expected verdicts and output bytes (tests/open_matrix_case.py):

  * result[i] is UINT64_MAX exactly on the damaged records and the claimed length on the intact ones;
  * the claimed-length output bytes of every record, damaged ones included, are the oracle's (decrypt-then-verify);
  * every other byte of `out` is still 0xA5; in place (in == out) the 16 tag bytes after each record are unchanged.

Shapes: L = 16 (5 G + 1) + 5, A = 21 at G lanes per record (two iterations of the full-block stretch, a generic element
per lane, a 5-byte partial block, lanes shifted by two AAD blocks); lanes = 64 (the sparse kernel) at N = 41 and 154
GHASH elements with a key per record; the tiny shapes (L, A) = (0, 0), (0, 21), (1, 0), (16, 16).  tests/test_open_matrix_ref.py
checks the same lists against the references alone.

The same matrix run on the TEST-ONLY mutant build (batch_kernel.h OPEN_MUTANT 1: the tag compare ignores tag bytes 8..11
at G = 8 and 32) must report exactly tag bits 64..95 accepted, so the matrix is known to see the verdict path break.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import open_matrix as om  # noqa: E402
import open_matrix_case as omc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MUTANT = os.path.join(os.path.dirname(HERE), "hsig-picotls_amd", "mutants", "libptls_hip_open1.so")
BATCH_GS = [1, 2, 4, 8, 16, 32]


@pytest.mark.parametrize("align", [16, 1])
@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("lanes", BATCH_GS)
def test_batch_kernel(engine, oracle, lanes, key_len, align):
    omc.check(engine, oracle, omc.batch_cases(oracle, key_len, lanes), lanes, wg=768, align=align)


@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("lanes", [4, 32])
def test_batch_kernel_512_threads(engine, oracle, lanes, key_len):
    omc.check(engine, oracle, omc.batch_cases(oracle, key_len, lanes), lanes, wg=512, align=16)


@pytest.mark.parametrize("align", [16, 1])
@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("lanes", BATCH_GS + [64])
def test_tiny_shapes(engine, oracle, lanes, key_len, align):
    """records of 0, 1 and 16 bytes with AADs of 0, 16 and 21: every tag bit and the length cases that exist"""
    cases = omc.tiny_cases(oracle, key_len)
    assert {om.claimed_len(c) for c in cases if c.kind == "I"} == {0, 1, 16}
    omc.check(engine, oracle, cases, lanes, align=align)


@pytest.mark.parametrize("align", [16, 1])
@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("n_elements", omc.SPARSE_N)
def test_sparse_kernel(engine, oracle, n_elements, key_len, align):
    """lanes = 64, every record under a key of its own"""
    omc.check(engine, oracle, omc.sparse_cases(oracle, key_len, n_elements), 64, align=align)


@pytest.mark.parametrize("align", [16, 1])
@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("lanes", BATCH_GS + [64])
def test_open_in_place(engine, oracle, lanes, key_len, align):
    """in == out: the plaintext replaces the ciphertext, the tag behind it and the bytes between the records stay.  align 1
    packs the records, so a record's last block is followed at once by its tag and the next record's first block"""
    cases = (omc.batch_cases(oracle, key_len, lanes) if lanes < 64 else omc.sparse_cases(oracle, key_len, 154)) + \
        omc.tiny_cases(oracle, key_len)
    _, out = omc.check(engine, oracle, cases, lanes, align=align, in_place=True)
    pos = 0
    for c in cases:  # (the whole-buffer compare above covers this; stated on its own because it is the contract)
        pos = (pos + align - 1) // align * align
        assert out[pos + om.claimed_len(c): pos + len(c.sealed)].tobytes() == c.sealed[-16:]
        pos += len(c.sealed)


def _mutant_run(lanes):
    if not os.path.exists(MUTANT):
        pytest.fail(f"{MUTANT} missing: build it with `make -C hsig-picotls_amd mutants` (part of __graft_entry__.build())")
    env = dict(os.environ, PTLS_HIP_LIB=MUTANT)
    out = subprocess.run([sys.executable, os.path.join(HERE, "open_matrix_case.py"), str(lanes), "16"], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = next(ln for ln in out.stdout.splitlines() if ln.startswith("MISMATCHES"))
    assert MUTANT in line, line
    return {k: v for k, v in (f.split("=", 1) for f in line.split()[1:])}


@pytest.mark.parametrize("lanes", [8, 32])
def test_open_mutant_is_caught(lanes):
    """the tag compare without tag bytes 8..11: exactly the 32 tag bits of those bytes are accepted, nothing else is wrong"""
    got = _mutant_run(lanes)
    assert sorted(got["accepted"].split(",")) == sorted(f"T:{bit}" for bit in range(64, 96)), got
    assert (got["rejected"], got["other"], got["bytes"]) == ("", "", "0"), got
