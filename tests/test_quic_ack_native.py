"""The rule of hsig-picotls_amd/csrc/quic_ack.h, the code quic_ack_kernel.hip runs, compiled with plain g++ into a
stand-alone program (tests/native/quic_ack_check.cpp, no GPU, no HIP call) and checked byte for byte against the plain-Python
model (tests/quic_ack_ref.py).

The grid is tests/quic_ack_cases.py's: next at 0, 1, the window's edges, every varint edge of the largest acknowledged, 2^62
and past it, against windows that are full, a single bit, alternating (31 further ranges), bit 0 clear and stray above next;
crossed with the delay at every varint edge and max_ranges 0, 1, 30, 31, 32 and 2^32 - 1; 4 000 random windows from a fixed
seed; and whole calls (the case list per space, lists of 1 .. 2 049 entries, all-empty, the 5 / 74 and 12 / 81 byte
neighbours), which the program walks in forward and in backward entry order.

The same program is built a second time with AddressSanitizer and UndefinedBehaviorSanitizer and run stand-alone over the
same cases: it must exit clean (every frame buffer there has exactly the bytes the model wants)."""
import os
import shutil
import subprocess

import pytest

import quic_ack_cases as gen
import quic_ack_ref as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hsig-picotls_amd", "csrc")
NEEDS = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _entry_line(n, w, delay, keep):
    st = model.status(0, 1, n, w)
    f = model.frame(n, w, delay, keep) if st == model.OK else b""
    return "F %d %d %d %d %d %s\n" % (n, w, delay, keep, st, f.hex() or "-"), st, len(f)


def _call_line(call):
    o = call.want()
    words = [call.count, call.space, call.ack_delay, call.max_ranges, call.in_off, call.pkt_base, call.pkt_stride, len(call.conns)]
    words += [x for s in call.spaces for x in s] + call.conns + o.status + o.frame_off + o.frame_len + [len(o.reqs)]
    words += [x for r in o.reqs for x in r]
    return "C " + " ".join(str(w) for w in words) + " " + (o.bytes.hex() or "-") + "\n", o


def _lines():
    lines, statuses, lengths = [], set(), set()
    for n, w in gen.grid() + gen.stray_bits():
        for delay in gen.DELAYS:
            for keep in gen.MAX_RANGES if delay in (0, (1 << 62) - 1) else (31,):
                line, st, size = _entry_line(n, w, delay, keep)
                lines.append(line)
                statuses.add(st)
                lengths.add(size)
    for k, (n, w) in enumerate(gen.random_entries(4000, seed=7)):
        lines.append(_entry_line(n, w, gen.DELAYS[k % len(gen.DELAYS)], 31 if k % 3 else k % 40)[0])
    assert statuses == {model.OK, model.EMPTY, model.STATE} and {0, 5, 81} <= lengths
    seen = set()
    for space in range(3):
        for kw in (dict(), dict(ack_delay=(1 << 62) - 1, max_ranges=1, in_off=(1 << 64) - 1 - 81 * 150, pkt_base=1 << 40, pkt_stride=1 << 50)):
            line, o = _call_line(gen.case_list(space, **kw))
            lines.append(line)
            seen |= set(o.status)
        lines.append(_call_line(gen.case_list(space).permuted(space + 5))[0])
    assert seen == {model.OK, model.NO_CONN, model.EMPTY, model.STATE}
    for n in (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049):
        lines.append(_call_line(gen.sized_call(n, pkt_stride=100))[0])
    lines.append(_call_line(gen.empty_call())[0])
    for delay, want in ((0, {5, 74}), ((1 << 62) - 1, {12, 81})):
        line, o = _call_line(gen.edge_call(delay))
        assert set(o.frame_len) == want
        lines.append(line)
    return lines


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("quic_ack") / "cases.txt"
    lines = _lines()
    assert len(lines) > 12000
    with open(path, "w") as f:
        f.writelines(lines)
    return path, len(lines)


def _build(exe, extra):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC, *extra,
                    os.path.join(ROOT, "tests", "native", "quic_ack_check.cpp"), "-o", str(exe)], check=True)


@NEEDS
def test_quic_ack_rule_matches_the_model(cases, tmp_path):
    path, n = cases
    exe = tmp_path / "quic_ack_check"
    _build(exe, [])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(n)], r.stdout[-2000:] + r.stderr[-2000:]


@NEEDS
def test_quic_ack_rule_under_sanitizers(cases, tmp_path):
    """the same program with ASan + UBSan, run stand-alone (no preloaded runtime): it exits clean"""
    path, n = cases
    exe = tmp_path / "quic_ack_check_san"
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(n)], out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
