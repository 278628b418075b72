"""The arithmetic of the device-side receive step (hsig-picotls_amd/csrc/quic_rx.h, the code quic_rx_kernel.hip runs) and the
host planning behind it (planner.cpp, slice_plan.cpp's quic_records), linked into a stand-alone program with plain g++
(tests/native/quic_rx_check.cpp, no GPU, no HIP call) and checked against the plain-Python model (tests/quic_rx_ref.py).

The select rule, over a few thousand descriptors: every boundary of the rule on its own against an otherwise good descriptor
(pkt_len = pn_offset + 19 / 20, 65535 / 65536, a packet that ends at buf_len - 1 / buf_len / buf_len + 1, a plaintext area that
ends at out_len - 1 / out_len / out_len + 1, key and hp_key at nslots - 1 / nslots / 0xffffffff, each type bit set and clear,
with and without info records, offsets that would wrap 64 bits), then random combinations of the boundary values.

Packet lists: the model's sums, lanes and plan order against the program's three ways to them (see its header): interleaved
connections (the wave-per-record kernel), long key runs of short and long packets (every batch-kernel width), lengths on the
16-byte block boundaries with many ties, already sorted lists.

The same program is built a second time with AddressSanitizer and UndefinedBehaviorSanitizer and run stand-alone over the
same cases: it must exit clean."""
import itertools
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import quic_rx_ref as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hsig-picotls_amd", "csrc")
NEEDS = pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"),
                           reason="needs g++ and the HIP headers")
PKT = np.dtype([("pkt_off", "<u8"), ("data_off", "<u8"), ("pn", "<u8"), ("pkt_len", "<u4"), ("key", "<u4"), ("hp_key", "<u4"),
                ("pn_offset", "<u2"), ("pn_len", "u1"), ("flags", "u1")])
BUF, OUT, NSLOTS, HP_NSLOTS = 100000, 90000, 64, 48
GOOD = dict(pkt_off=1000, data_off=2000, pkt_len=300, key=5, hp_key=6, pn_offset=9, type=4)

# per field: the values on both sides of every limit of the rule
BOUNDARY = {
    "pn_offset": [0, 1, 9, 47, 280, 281, 65535],
    "pkt_len": [0, 9 + 19, 9 + 20, 300, 65535, 65536, 0xFFFFFFFF],
    "pkt_off": [0, BUF - 301, BUF - 300, BUF - 299, BUF, BUF + 1, (1 << 64) - 1, (1 << 64) - 300],
    "data_off": [0, OUT - 275, OUT - 274, OUT - 273, OUT, OUT + 1, (1 << 64) - 1, (1 << 64) - 274],
    "key": [0, NSLOTS - 1, NSLOTS, 0xFFFFFFFF],
    "hp_key": [0, HP_NSLOTS - 1, HP_NSLOTS, 0xFFFFFFFF],
    "type": [0, 1, 2, 3, 4, 5, 6, 7, 31, 32, 255],
}
MASKS = [0xFF, 0, 1 << 4, 1 << 2, 0x17, 0xFFFFFFFF, 1 << 31]


def _select_lines():
    rng = random.Random(91)
    lines, wanted = [], []

    def emit(d, mask, has_info, buf=BUF, out=OUT):
        want = model.selectable(d, d["type"], buf, out, NSLOTS, HP_NSLOTS, mask, bool(has_info))
        wanted.append(want)
        lines.append("S %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n" % (
            buf, out, NSLOTS, HP_NSLOTS, mask, has_info, d["pkt_off"], d["data_off"], d["pkt_len"], d["key"], d["hp_key"],
            d["pn_offset"], d["type"], int(want)))

    for field, values in BOUNDARY.items():  # one field at its boundaries, the rest good
        for v, mask, has_info in itertools.product(values, MASKS, (0, 1)):
            emit(dict(GOOD, **{field: v}), mask, has_info)
    assert model.selectable(dict(GOOD, pkt_len=29), 4, BUF, OUT, NSLOTS, HP_NSLOTS) and \
        not model.selectable(dict(GOOD, pkt_len=28), 4, BUF, OUT, NSLOTS, HP_NSLOTS)
    assert model.selectable(dict(GOOD, pkt_off=BUF - 300), 4, BUF, OUT, NSLOTS, HP_NSLOTS) and \
        not model.selectable(dict(GOOD, pkt_off=BUF - 299), 4, BUF, OUT, NSLOTS, HP_NSLOTS)
    assert model.selectable(dict(GOOD, data_off=OUT - 274), 4, BUF, OUT, NSLOTS, HP_NSLOTS) and \
        not model.selectable(dict(GOOD, data_off=OUT - 273), 4, BUF, OUT, NSLOTS, HP_NSLOTS)
    for buf, out in ((0, 0), (300, 274), (299, 274), (300, 273), ((1 << 64) - 1, (1 << 64) - 1)):  # the smallest buffers
        emit(dict(GOOD, pkt_off=0, data_off=0), 0xFF, 1, buf, out)
    for _ in range(3000):  # combinations
        d = {f: rng.choice(v) for f, v in BOUNDARY.items()}
        if rng.randrange(3):
            d["pkt_len"] = rng.choice((d["pn_offset"] + 19, d["pn_offset"] + 20, d["pn_offset"] + 400))
        if rng.randrange(2):
            d = dict(GOOD, **{f: d[f] for f in rng.sample(sorted(d), 2)})
        emit(d, rng.choice(MASKS), rng.randrange(2))
    assert 300 < sum(wanted) < len(wanted) - 300
    return lines


def _list(rng, n, nkeys, run, length):
    """n packets, keys in runs of `run` over nkeys connections, lengths from length(rng)"""
    p = np.zeros(n, dtype=PKT)
    p["pn_offset"] = [rng.choice((1, 9, 18, 21, 47)) for _ in range(n)]
    p["pkt_len"] = [int(po) + 17 + length(rng) for po in p["pn_offset"]]
    p["key"] = [(i // run) % nkeys for i in range(n)]
    return p


def _lists():
    rng = random.Random(92)
    ties = lambda r: r.choice((3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 255, 256, 257))  # noqa: E731
    out = []
    for ncu in (256, 8):
        out += [(ncu, _list(rng, 1, 1, 1, ties)), (ncu, _list(rng, 2, 2, 1, ties)),
                (ncu, _list(rng, 1000, 64, 1, ties)),                                  # interleaved: sparse
                (ncu, _list(rng, 1000, 64, 19, ties)), (ncu, _list(rng, 1000, 64, 20, ties)),  # the sparse threshold
                (ncu, _list(rng, 3000, 1, 3000, lambda r: r.randrange(3, 1400))),
                (ncu, _list(rng, 640, 10, 64, lambda r: r.randrange(4200, 16000))),    # long records, short runs: 32 lanes
                (ncu, _list(rng, 1280, 10, 128, lambda r: r.randrange(4200, 16000))),  # 16
                (ncu, _list(rng, 3000, 10, 300, lambda r: r.randrange(4200, 16000))),  # 8
                (ncu, _list(rng, 64, 1, 64, lambda r: 1200)),                          # equal lengths on one key
                (ncu, _list(rng, 2000, 1, 2000, lambda r: 300)), (ncu, _list(rng, 2000, 1, 2000, lambda r: 40)),  # 2 lanes, 1 lane
                (ncu, _list(rng, 500, 500, 1, lambda r: r.randrange(3, 65000)))]
        srt = _list(rng, 700, 70, 1, ties)
        srt = srt[np.argsort(-model.lens(srt), kind="stable")]                         # already in plan order
        out.append((ncu, srt))
    for _ in range(40):
        n = rng.randrange(1, 2500)
        out.append((rng.choice((256, 64, 304)), _list(rng, n, rng.randrange(1, 80), rng.choice((1, 2, 7, 19, 20, 21, 64, 400)),
                                                      rng.choice((ties, lambda r: r.randrange(3, 1500), lambda r: r.randrange(3, 9000))))))
    return out


def _list_lines():
    lines, seen, lists = [], set(), _lists()
    for ncu, p in lists:
        ghash, blocks, runs, max16, n = model.stats(p)
        lanes, chacha = model.choose_lanes(ghash, runs, n, ncu), model.choose_chacha_lanes(blocks, n, ncu)
        seen.add(lanes)
        lines.append("L %d %d %d %d %d %d %d %d\n" % (ncu, n, ghash, blocks, runs, max16, lanes, chacha))
        lines += ["%d %d %d\n" % (a, b, c) for a, b, c in zip(p["pkt_len"], p["pn_offset"], p["key"])]
        lines.append(" ".join(map(str, model.plan_order(p).tolist())) + "\n")
    assert seen >= {64, 32, 16, 8, 4, 2, 1}, seen
    return lines, len(lists)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("quic_rx") / "cases.txt"
    sel = _select_lines()
    lst, nlists = _list_lines()
    assert len(sel) >= 3000
    with open(path, "w") as f:
        f.writelines(sel + lst)
    return path, len(sel) + nlists


def _build(exe, extra):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, *extra, os.path.join(ROOT, "tests", "native", "quic_rx_check.cpp"),
                    os.path.join(CSRC, "planner.cpp"), os.path.join(CSRC, "slice_plan.cpp"), "-o", str(exe)], check=True)


@NEEDS
def test_quic_rx_arithmetic_matches_the_model(cases, tmp_path):
    path, n = cases
    exe = tmp_path / "quic_rx_check"
    _build(exe, [])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(n)], r.stdout[-2000:] + r.stderr[-2000:]


@NEEDS
def test_quic_rx_arithmetic_under_sanitizers(cases, tmp_path):
    """the same program with ASan + UBSan, run stand-alone (no preloaded runtime): it exits clean"""
    path, n = cases
    exe = tmp_path / "quic_rx_check_san"
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(n)], out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
