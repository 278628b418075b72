"""The copy transport's planning of QUIC packet slices (hsig-picotls_amd/csrc/slice_plan.cpp: quic_records and
plan_quic_slice over plan_copy_slice), linked into a stand-alone program with plain g++ (tests/native/quic_slice_check.cpp,
no GPU, no HIP call) and run over more than 2 000 seeded packet lists, for seal and for open.

This file generates the lists and its own model of the plan: the greedy cut (a slice grows while the span of its packets'
input and the span of its output fit slice_bytes each and it holds at most slice_bytes / 64 packets) and the refusal of a
packet that does not fit a slice.  The program compares the cut and checks every slice on byte maps of the caller's buffers
(see its header): staging limits, slice-local offsets that keep the caller's alignment modulo 16, the header pieces (seal),
the copies back and the filled gaps, the staged tails of the plaintext areas at their pn_len = 1 length (open).

The lists: packets of 21 to 1 500 bytes 1 to 64 bytes apart, in order and shuffled, pn_offset 1 to 47, every pn_len; tiny
packets (21 to 24 bytes) by the thousand, which end slices at the packet cap; long lists of MTU-sized packets, whose slices
hold more runs than are copied one by one (the gap-filled copies); a packet of exactly slice_bytes, and one of one byte
more, which is refused.

The same program is built a second time with AddressSanitizer and UndefinedBehaviorSanitizer and run stand-alone over the
same cases: it must exit clean."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hsig-picotls_amd", "csrc")
SLICE = 64 << 10
NEEDS = pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"),
                           reason="needs g++ and the HIP headers")


def _packet(rng, kind):
    pn_offset = rng.choice((1, 9, 18, 21, 47)) if kind != "tiny" else 1
    pn_len = rng.randrange(1, 5)
    if kind == "tiny":
        payload = 20 - pn_offset - pn_len - 16 + rng.randrange(1, 5)  # pkt_len 21 .. 24
        payload = max(payload, 4 - pn_len)
    elif kind == "mtu":
        payload = rng.choice((1200, 1350, 1452))
    else:
        payload = rng.choice((0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 1200, 1350, rng.randrange(0, 1500)))
        payload = max(payload, 4 - pn_len)  # the sample at pn_offset + 4 ends inside the packet
    return pn_offset, pn_len, pn_offset + pn_len + payload + 16


def _place(rng, sizes):
    offs, pos = [], 0
    for s in sizes:
        pos += rng.randrange(1, 65)
        offs.append(pos)
        pos += s
    return offs


def _list(rng, n, kind, shuffled, is_open, lens=None):
    """packets as (pkt_off, data_off, pkt_len, pn_offset, pn_len, flags), in descriptor order"""
    shape = [_packet(rng, kind) for _ in range(n)]
    if lens is not None:
        shape = [(1, pl, L) for (_, pl, _), L in zip(shape, lens)]
    pkt_offs = _place(rng, [s[2] for s in shape])
    if is_open:
        data_offs = _place(rng, [L - po - 17 for po, _, L in shape])  # the pn_len = 1 areas
    elif rng.randrange(4) == 0:
        data_offs = [o + po + pl for o, (po, pl, _) in zip(pkt_offs, shape)]  # in place
    else:
        data_offs = _place(rng, [L - po - pl - 16 for po, pl, L in shape])
    pk = [(pkt_offs[i], data_offs[i], shape[i][2], shape[i][0], shape[i][1], rng.randrange(2) if is_open else 0) for i in range(n)]
    if shuffled:
        rng.shuffle(pk)
    return pk


def _model_cut(pk, is_open, slice_bytes):
    """(ends of the slices, index of the refused packet or None): the greedy cut"""
    cap = slice_bytes // 64
    ends, i, n = [], 0, len(pk)
    while i < n:
        in_lo = out_lo = None
        j = i
        while j < n and j - i < cap:
            pkt_off, data_off, pkt_len, pn_offset, pn_len, _ = pk[j]
            if is_open:
                a = (pkt_off, pkt_off + pkt_len)
                b = (data_off, data_off + pkt_len - pn_offset - 17)
            else:
                a = (data_off, data_off + pkt_len - pn_offset - pn_len - 16)
                b = (pkt_off, pkt_off + pkt_len)
            if j == i:
                ni, no = a, b
            else:
                ni = (min(in_lo, a[0]), max(in_hi, a[1]))
                no = (min(out_lo, b[0]), max(out_hi, b[1]))
                if ni[1] - ni[0] > slice_bytes or no[1] - no[0] > slice_bytes:
                    break
            (in_lo, in_hi), (out_lo, out_hi) = ni, no
            j += 1
        if in_hi - in_lo > slice_bytes or out_hi - out_lo > slice_bytes:
            return ends, i
        ends.append(j)
        i = j
    return ends, None


def _cases():
    rng = random.Random(20261020)
    out = []
    for k in range(2000):
        is_open = k % 2 == 1
        out.append((is_open, SLICE, _list(rng, rng.randrange(1, 140), "mixed", k % 4 >= 2, is_open)))
    for k in range(8):  # the packet cap: more than slice_bytes / 64 tiny packets per slice
        out.append((k % 2 == 1, SLICE, _list(rng, 2600, "tiny", k >= 4, k % 2 == 1)))
    for k in range(24):  # many runs per slice: the gap-filled copies
        out.append((k % 2 == 1, SLICE if k % 3 else 1 << 20, _list(rng, 400, "mtu", k % 4 >= 2, k % 2 == 1)))
    for k in range(8):  # a packet of exactly a slice, between others; and one byte more: refused at that packet
        for extra in (0, 1):
            is_open = k % 2 == 1
            lens = [300, 1400, SLICE + extra, 700, 21]
            out.append((is_open, SLICE, _list(rng, 5, "mixed", False, is_open, lens=lens)))
    return out


def _write(path):
    cases = _cases()
    refused = caps = exact = 0
    with open(path, "w") as f:
        for cid, (is_open, slice_bytes, pk) in enumerate(cases):
            ends, bad = _model_cut(pk, is_open, slice_bytes)
            refused += bad is not None
            caps += any(b - a == slice_bytes // 64 for a, b in zip([0] + ends, ends))
            exact += bad is None and any(p[2] == slice_bytes for p in pk)
            f.write("C %d %s %d %d %d %d\n" % (cid, "O" if is_open else "S", slice_bytes, len(pk), -1 if bad is not None else len(ends),
                                               bad if bad is not None else 0))
            for p in pk:
                f.write("%d %d %d %d %d %d\n" % p)
            f.write(" ".join(map(str, ends)) + "\n")
    assert len(cases) >= 2000 and refused == 8 and exact == 8 and caps >= 4, (len(cases), refused, exact, caps)
    return len(cases)


def _build(exe, extra):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, *extra, os.path.join(ROOT, "tests", "native", "quic_slice_check.cpp"),
                    os.path.join(CSRC, "slice_plan.cpp"), "-o", str(exe)], check=True)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("quic_slice") / "cases.txt"
    return path, _write(path)


@NEEDS
def test_quic_slice_plans(cases, tmp_path):
    path, n = cases
    exe = tmp_path / "quic_slice_check"
    _build(exe, [])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[:2] == ["ok", str(n)], r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[2]) > n  # most lists are cut into several slices


@NEEDS
def test_quic_slice_plans_under_sanitizers(cases, tmp_path):
    """the same program with ASan + UBSan, run stand-alone (no preloaded runtime): it exits clean"""
    path, n = cases
    exe = tmp_path / "quic_slice_check_san"
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.split()[:2] == ["ok", str(n)], out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
