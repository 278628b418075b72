"""The rule of hsig-picotls_amd/csrc/quic_tx.h, the code quic_tx_kernel.hip runs, compiled with plain g++ into a stand-alone
program (tests/native/quic_tx_check.cpp, no GPU, no HIP call) and checked against the plain-Python model
(tests/quic_tx_ref.py).

The grid is tests/quic_tx_cases.py's: the case list (RFC 9000 A.2's examples, every boundary of the packet-number length, the
end of the number space, acknowledged numbers, connection-ID lengths 0 / 8 / 20 / 21, payloads too short for the sample, the
packet-length limit, offsets at and past both buffers' ends, connections outside each of the three bounds, second runs, the
precedence of the refusals, four generations) for params.pn_len 0 .. 4, with receive-side generations below, at and above the
send side's, with smaller state counts, strides and header-protection keysets; the size calls of the GPU test; and the length
function alone around every threshold.  The program walks the passes single-threaded in forward and in backward request
order.

The same program is built a second time with AddressSanitizer and UndefinedBehaviorSanitizer and run stand-alone over the
same cases: it must exit clean."""
import os
import shutil
import subprocess

import pytest

import quic_tx_cases as gen
import quic_tx_ref as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hsig-picotls_amd", "csrc")
NEEDS = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def call_line(call):
    o = call.want()
    words = [call.count, call.stride, call.hp_slots, call.in_len, call.buf_len, call.pn_len, int(call.rx_gens is not None), len(call.reqs)]
    for c in range(call.count):
        k = call.conns[c]
        words += [k.next_pn, k.largest_acked, k.gen, k.dcid_len, k.flags, k.dcid.ljust(20, b"\xee").hex(),
                  call.rx_gens[c] if call.rx_gens is not None else 0]
    words += [x for r in call.reqs for x in r]
    for j in range(len(call.reqs)):
        sent = o.status[j] == model.SENT
        words += [o.status[j], o.pn_out[j], o.pkt_len[j], o.slots[j] if sent else -1, o.headers[j].hex() if sent else "-"]
    for c in range(call.count):
        words += [o.conns[c].next_pn, o.conns[c].gen]
    return "C " + " ".join(str(w) for w in words) + "\n", o


def _lines():
    lines, seen = [], set()
    for la in (model.NONE_ACKED, 0, 1000, 0xabe8b3, (1 << 62) - (1 << 31) - 5):
        for k in (7, 15, 23, 31):
            for d in (-2, -1, 0, 1):
                unacked = (1 << k) + d
                pn = unacked - 1 if la == model.NONE_ACKED else la + unacked
                for min_len in range(5):
                    lines.append("L %d %d %d %d\n" % (pn, la, min_len, model.pn_len(pn, la, min_len)))
    for pn_len in range(5):
        for rx in (None, "mixed"):
            call = gen.case_list(pn_len, rx)
            for variant in (call, call.with_(count=60), call.with_(stride=100), call.with_(hp_slots=7)):
                line, o = call_line(variant)
                lines.append(line)
                seen |= set(o.status)
    assert seen == {model.SENT, model.NO_CONN, model.SPLIT, model.PN, model.RANGE}
    for call in (gen.sized_call(1), gen.sized_call(255), gen.sized_call(257), gen.sized_call(2049), gen.one_run_call(4096),
                 gen.edges_call(), gen.many_runs_call(2047), gen.many_runs_call(2049), gen.lengths_call()):
        lines.append(call_line(call)[0])
    return lines


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("quic_tx") / "cases.txt"
    lines = _lines()
    assert len(lines) > 400
    with open(path, "w") as f:
        f.writelines(lines)
    return path, len(lines)


def _build(exe, extra):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, *extra, os.path.join(ROOT, "tests", "native", "quic_tx_check.cpp"), "-o", str(exe)], check=True)


@NEEDS
def test_quic_tx_rule_matches_the_model(cases, tmp_path):
    path, n = cases
    exe = tmp_path / "quic_tx_check"
    _build(exe, [])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(n)], r.stdout[-2000:] + r.stderr[-2000:]


@NEEDS
def test_quic_tx_rule_under_sanitizers(cases, tmp_path):
    """the same program with ASan + UBSan, run stand-alone (no preloaded runtime): it exits clean"""
    path, n = cases
    exe = tmp_path / "quic_tx_check_san"
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(n)], out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
