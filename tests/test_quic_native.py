"""The header arithmetic quic_kernel.hip runs (hsig-picotls_amd/csrc/quic.h), compiled for the host with plain g++ (no GPU)
and run as a stand-alone program (tests/native/quic_header_check.cpp) over more than 10 000 cases whose expected values come
from the plain-Python reference (tests/quic_ref.py):

  * the packet-number decode of RFC 9000 A.3 for every pn_len, expected values 0, 1, around half a window and a window,
    around 2^31 and 2^32 and just below 2^62, and truncated values at both edges of the decode window (candidate +- half a
    window, where the +- 2^(8 pn_len) corrections switch on) including the two guards that suppress the corrections
    (candidate < window near zero, candidate >= 2^62 - window at the top), plus random pairs;
  * applying a mask to a header and removing it, long and short first bytes, every pn_len, random masks, with a guard
    region behind the packet-number field that must come back unchanged."""
import os
import random
import shutil
import subprocess

import pytest

import quic_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PN_MAX = 1 << 62


def _decode_cases(rng):
    for pn_len in (1, 2, 3, 4):
        win = 1 << (8 * pn_len)
        hwin, mask = win // 2, win - 1
        base = [0, 1, 2, hwin - 1, hwin, hwin + 1, win - 1, win, win + 1, win + hwin - 1, win + hwin, win + hwin + 1,
                (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 32) + hwin,
                0xa82f30eb, PN_MAX - win - hwin - 1, PN_MAX - win - hwin, PN_MAX - win - 1, PN_MAX - win, PN_MAX - win + 1,
                PN_MAX - hwin - 1, PN_MAX - hwin, PN_MAX - hwin + 1, PN_MAX - 2, PN_MAX - 1, PN_MAX]
        for expected in base + [rng.randrange(PN_MAX) for _ in range(20)]:
            deltas = [-hwin - 1, -hwin, -hwin + 1, -2, -1, 0, 1, 2, hwin - 1, hwin, hwin + 1]
            truncs = {(expected + d) & mask for d in deltas} | {0, 1, mask, mask - 1, hwin, hwin - 1}
            truncs |= {rng.randrange(win) for _ in range(4)}
            for t in sorted(truncs):
                yield expected, t, pn_len
    for _ in range(3000):
        pn_len = rng.randrange(1, 5)
        yield rng.randrange(PN_MAX + 1), rng.randrange(1 << (8 * pn_len)), pn_len


def _header_cases(rng, count):
    for k in range(count):
        pn_len = k % 4 + 1
        pn_offset = (1, 9, 18, 21, 47)[k % 5] if k % 3 else rng.randrange(1, 300)
        h = bytearray(rng.randbytes(pn_offset + 4 + 1))
        h[0] = (h[0] & 0x7c) | (0x80 if k % 2 else 0) | (pn_len - 1)
        if k % 11 == 0:
            h[0] |= 0x1c  # every reserved / key-phase bit set
        mask = rng.randbytes(5) if k % 13 else bytes([0xff] * 5)
        yield bytes(h), pn_offset, pn_len, mask


def _write_cases(path):
    rng = random.Random(9000)
    n = 0
    with open(path, "w") as f:
        for expected, t, pn_len in _decode_cases(rng):
            f.write("D %d %d %d %d\n" % (expected, t, pn_len, quic_ref.decode_pn(expected, t, pn_len)))
            n += 1
        for h, pn_offset, pn_len, mask in _header_cases(rng, 3000):
            want = quic_ref.apply_mask(h[:pn_offset + pn_len], pn_offset, pn_len, mask) + h[pn_offset + pn_len:]
            f.write("P %d %d %s %s %s\n" % (pn_offset, pn_len, mask.hex(), h.hex(), want.hex()))
            n += 1
        for h, pn_offset, _, mask in _header_cases(rng, 3000):
            for masked in (1, 0):
                m = mask if masked else bytes(5)
                first = h[0] ^ (m[0] & quic_ref.first_byte_bits(h[0]))
                pn_len = (first & 3) + 1
                want = quic_ref.apply_mask(h[:pn_offset + pn_len], pn_offset, pn_len, m) + h[pn_offset + pn_len:]
                trunc = int.from_bytes(want[pn_offset: pn_offset + pn_len], "big")
                f.write("U %d %d %s %s %s %d %d\n" % (pn_offset, masked, mask.hex(), h.hex(), want.hex(), pn_len, trunc))
                n += 1
    return n


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_quic_header_functions_match_reference(tmp_path):
    exe = tmp_path / "quic_header_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "hsig-picotls_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "quic_header_check.cpp"), "-o", str(exe)], check=True)
    data = tmp_path / "cases.txt"
    n = _write_cases(data)
    assert n >= 10000
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == f"ok {n}", r.stdout + r.stderr
