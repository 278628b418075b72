"""The arithmetic chacha_kernel.hip runs (hsig-picotls_amd/csrc/chacha20.h, poly1305.h), compiled for the host (no GPU) and
run as a stand-alone program (tests/native/chacha_poly_check.cpp): the RFC 8439 §2.3.2 block, every Poly1305 vector of
Appendix A.3 (#1 - #11), and 2 000 (r, s, message) triples whose tags come from the big-integer reference
(tests/chacha_ref.py).  Every message is folded serially and through the kernel's lane split and combination for G = 1, 4,
16 and 64; the messages have 0 .. 3 * 4 * 64 + 5 whole blocks (so every G sees 0 .. 3 * 4G + 5 and more) and, every other
one, a partial last block.  Random records through the AEAD almost never reach an accumulator >= p, a limb carry chain of
all ones or the clamped bits of r, because r comes out of ChaCha: the A.3 vectors and the all-ones triples here do."""
import os
import random
import shutil
import struct
import subprocess

import pytest

import chacha_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTRIPLES = 2000
MAX_BLOCKS = 3 * 4 * 64 + 5


def _triples():
    rng = random.Random(8439)
    for i in range(NTRIPLES):
        nblocks = i % (MAX_BLOCKS + 1)
        n = 16 * nblocks + (rng.randrange(1, 16) if i % 2 else 0)
        kind = i % 7
        if kind == 0:  # the largest clamped r, all-ones message: long carry chains
            r, s, msg = b"\xff" * 16, b"\xff" * 16, b"\xff" * n
        elif kind == 1:  # small r: the accumulator stays near the blocks' values (>= 2^128, close to p after few steps)
            r, s, msg = bytes([rng.randrange(1, 4)]) + b"\x00" * 15, rng.randbytes(16), b"\xff" * n
        else:
            r, s, msg = rng.randbytes(16), rng.randbytes(16), rng.randbytes(n)
        yield r, s, msg


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_chacha_poly_headers_match_reference(tmp_path):
    exe = tmp_path / "chacha_poly_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "hsig-picotls_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "chacha_poly_check.cpp"), "-o", str(exe)], check=True)
    data = tmp_path / "triples.bin"
    with open(data, "wb") as f:
        for r, s, msg in _triples():
            f.write(r + s + struct.pack("<I", len(msg)) + msg + chacha_ref.poly1305_mac(msg, r + s))
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == f"ok {NTRIPLES}", r.stdout + r.stderr
