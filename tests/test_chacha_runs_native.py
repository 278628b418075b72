"""The piece map and quad transpose of chacha_runs_kernel.hip (hsig-picotls_amd/csrc/chacha_runs.h), compiled for the host (no
GPU) and run as a stand-alone program (tests/native/chacha_runs_check.cpp).  For G = 4, 16, 64 and every count of whole blocks
0 .. 3 G + 5: the pieces the lanes move are exactly the record's whole blocks, each once and none outside (the kernel's bounds);
every instruction moves one contiguous run per group; after the transpose each lane holds the block at place lambda(l).  Then
500 (r, s, message) triples whose tags come from the big-integer reference (tests/chacha_ref.py) are folded through that deal,
the accumulator permutation and the lane combination of poly1305.h: the all-ones triples of test_chacha_poly_native.py among
them, 0 .. 59 whole chunks each plus the trip boundaries of G = 64.  The program runs a second time built with
AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import random
import shutil
import struct
import subprocess

import pytest

import chacha_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTRIPLES = 500
BIG = [63, 64, 65, 127, 128, 129, 191, 192, 193, 197]  # chunks: the trip boundaries of G = 64, up to 3 G + 5


def _triples():
    rng = random.Random(8439)
    for i in range(NTRIPLES):
        chunks = i % 60 if i < 480 else BIG[(i - 480) % len(BIG)]
        n = 64 * chunks + 16 * ((i // 60) % 4) + (rng.randrange(1, 16) if i % 2 else 0)
        kind = i % 7
        if kind == 0:  # the largest clamped r, all-ones message: long carry chains
            r, s, msg = b"\xff" * 16, b"\xff" * 16, b"\xff" * n
        elif kind == 1:  # small r: the accumulator stays near the blocks' values
            r, s, msg = bytes([rng.randrange(1, 4)]) + b"\x00" * 15, rng.randbytes(16), b"\xff" * n
        else:
            r, s, msg = rng.randbytes(16), rng.randbytes(16), rng.randbytes(n)
        yield r, s, msg


@pytest.fixture(scope="module")
def triples_file(tmp_path_factory):
    data = tmp_path_factory.mktemp("runs") / "triples.bin"
    with open(data, "wb") as f:
        for r, s, msg in _triples():
            f.write(r + s + struct.pack("<I", len(msg)) + msg + chacha_ref.poly1305_mac(msg, r + s))
    return data


def _build_and_run(tmp_path, triples_file, extra):
    exe = tmp_path / "chacha_runs_check"
    subprocess.run(["g++", "-std=c++17", "-O2", *extra, "-I", os.path.join(ROOT, "hsig-picotls_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "chacha_runs_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(triples_file)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == f"ok {NTRIPLES}", r.stdout + r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_runs_piece_map_and_deal_match_reference(tmp_path, triples_file):
    _build_and_run(tmp_path, triples_file, [])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_runs_check_under_sanitizers(tmp_path, triples_file):
    _build_and_run(tmp_path, triples_file, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
