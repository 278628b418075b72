"""The rule of hsig-picotls_amd/csrc/quic_track.h, the code quic_track_kernel.hip runs, compiled with plain g++ into a
stand-alone program (tests/native/quic_track_check.cpp, no GPU, no HIP call) and checked against the plain-Python model
(tests/quic_track_ref.py).

The grid is tests/quic_track_cases.py's: every state crossed with packet numbers at next - 1 - pn of 0, 1, 62 .. 65, shifts of
1, 63, 64, 65 and 2^40, and 2^62 - 1; alone, in every ordered pair (both orders of every duplicate pair), with a failed copy
in front, three times over; each in a table of three connections whose other spaces must not change, at the connection count - 1
and at count, with and without a short expected-pn table.  The program walks the three passes single-threaded in forward and
in backward packet order.  The probe functions alone are driven to a table that is exactly half full, with the hash's own
spread and with every key starting at one slot.

The same program is built a second time with AddressSanitizer and UndefinedBehaviorSanitizer and run stand-alone over the
same cases: it must exit clean."""
import os
import shutil
import subprocess

import pytest

import quic_track_cases as gen
import quic_track_ref as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hsig-picotls_amd", "csrc")
NEEDS = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _call_line(call, expected):
    verdicts, touched, after, exp = call.want(expected)
    words = [call.count, len(expected), len(call.packets)]
    words += [x for s in call.spaces for x in s] + list(expected) + [x for p in call.packets for x in p]
    words += verdicts + [x for s in after for x in s] + exp + [len(touched)] + touched
    return "T " + " ".join(str(w) for w in words) + "\n", verdicts


def _lines():
    lines, seen = [], set()
    for k, case in enumerate(gen.grid()):
        next_, window, pk = case
        for _, pn in pk:
            want = model.TOO_OLD if pn < next_ and next_ - 1 - pn >= 64 else \
                model.DUPLICATE if pn < next_ and pn in model.accepted(next_, window) else model.NONE
            lines.append("O %d %d %d %d\n" % (pn, next_, window, want))
        # the connection at count - 1 (tracked) and, every seventh case, at count (not tracked: nothing changes)
        conn = 3 if k % 7 == 3 else 2 if k % 2 else k % 3
        call = gen.single(case, count=3, conn=conn, space=k % 3) if conn < 3 else \
            gen.Call(3, [[77, 0b1011]] * 9, [(3, model.ONE_RTT, r, pn) for r, pn in pk])
        line, verdicts = _call_line(call, [900 + i for i in range((0, 9, 7, 12)[k % 4])])
        assert conn < 3 or set(verdicts) == {model.NONE}
        seen |= set(verdicts)
        lines.append(line)
    assert seen == {model.NONE, model.NEW, model.DUPLICATE, model.TOO_OLD}
    for part in range(3):
        call = gen.case_list(part)
        lines.append(_call_line(call, [0] * call.expected_len)[0])
        lines.append(_call_line(call.permuted(part), [])[0])
    for call in (gen.bulk_call(), gen.distinct_call(257), gen.copies_call(), gen.triples_call(), gen.seam_call(2049)):
        lines.append(_call_line(call, [5] * (3 * call.count))[0])
    for keys in (1, 2, 64, 1024):
        lines += ["P %d 0\n" % keys, "P %d 1\n" % keys]
    return lines


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("quic_track") / "cases.txt"
    lines = _lines()
    assert len(lines) > 30000
    with open(path, "w") as f:
        f.writelines(lines)
    return path, len(lines)


def _build(exe, extra):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC, *extra,
                    os.path.join(ROOT, "tests", "native", "quic_track_check.cpp"), "-o", str(exe)], check=True)


@NEEDS
def test_quic_track_rule_matches_the_model(cases, tmp_path):
    path, n = cases
    exe = tmp_path / "quic_track_check"
    _build(exe, [])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(n)], r.stdout[-2000:] + r.stderr[-2000:]


@NEEDS
def test_quic_track_rule_under_sanitizers(cases, tmp_path):
    """the same program with ASan + UBSan, run stand-alone (no preloaded runtime): it exits clean"""
    path, n = cases
    exe = tmp_path / "quic_track_check_san"
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(n)], out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
