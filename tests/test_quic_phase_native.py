"""The rule of hsig-picotls_amd/csrc/quic_phase.h, the code quic_phase_kernel.hip runs, compiled with plain g++ into a
stand-alone program (tests/native/quic_phase_check.cpp, no GPU, no HIP call) and checked against the plain-Python model
(tests/quic_phase_ref.py).

The choice: gen in {0 .. 6, 2^32 - 2} crossed with first_pn in {0, 1, pn - 1, pn, pn + 1, UINT64_MAX}, both Key Phase bits,
short and long first bytes with every value of the other protected bits, the header-protection mask present and absent
(PTLS_HIP_QUIC_UNPROTECTED: the byte as it stands), and the slot for strides and keys up to the 32-bit limits.  The commit: what
a packet counts as, and the state after it, around every boundary (failed, long header, generations gen - 1 .. gen + 2,
first_pn lowered, equal and not raised).

The same program is built a second time with AddressSanitizer and UndefinedBehaviorSanitizer and run stand-alone over the
same cases: it must exit clean."""
import itertools
import os
import random
import shutil
import subprocess

import pytest

import quic_phase_ref as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hsig-picotls_amd", "csrc")
NEEDS = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
U64, NO_GEN = model.U64, model.NO_GEN
GENS = [0, 1, 2, 3, 4, 5, 6, 2 ** 32 - 2]
PNS = [1, 2, 77, 1 << 32, (1 << 62) - 2]


def first_pns(pn):
    return [0, 1, pn - 1, pn, pn + 1, U64]


def _unmasked(first, masked, m0):
    return first ^ (m0 & (0x0f if first & 0x80 else 0x1f)) if masked else first


def _choice_lines():
    rng = random.Random(95)
    lines, outcomes = [], set()

    def emit(first, masked, m0, pn, gen, first_pn, key, stride):
        fb = _unmasked(first, masked, m0)
        g = model.choose(fb, pn, gen, first_pn)
        outcomes.add("long" if g == NO_GEN else g - gen)
        lines.append("G %d %d %d %d %d %d %d %d %d %d %d\n" % (first, masked, m0, pn, gen, first_pn, key, stride, fb, g,
                                                               model.slot(key, stride, g)))

    for gen, pn in itertools.product(GENS, PNS):
        for first_pn in first_pns(pn):
            for first in (0x40, 0x44, 0x5b, 0x5f, 0x00, 0x04, 0xc0, 0xc4, 0xef, 0xfb, 0x80):  # both bits; short and long
                emit(first, 0, 0xffffffff, pn, gen, first_pn, 5, 137)                        # the byte as it stands
                for m0 in (0, 0x04, 0x1f, 0xffffffe4, rng.getrandbits(32)):                   # the mask flips the bit or not
                    emit(first, 1, m0, pn, gen, first_pn, 5, 137)
    for key, stride in ((0, 1), (129, 130), (0, 0x55555555), (0x55555554, 0x55555555), (1, 1431655765)):
        for gen in GENS:
            emit(0x44, 0, 0, 9, gen, 9, key, stride)
            emit(0xc4, 0, 0, 9, gen, 9, key, stride)
    assert outcomes == {"long", -1, 0, 1}
    return lines


def _commit_lines():
    lines = []
    for gen in GENS:
        for gen_out in sorted({max(gen - 1, 0), gen, gen + 1, min(gen + 2, NO_GEN), 0, NO_GEN}):
            for result in (0, 1, 1200, U64 - 1, U64):
                want = 0 if result == U64 or gen_out == NO_GEN else 1 if gen_out == gen else 2 if gen_out == gen + 1 else 0
                t = [[gen, 50]]
                upd = model.commit(t, [0], [result], [7], [gen_out])
                assert (want == 2) == (upd == [0]) and (want == 1) == (t == [[gen, 7]])
                lines.append("C %d %d %d %d\n" % (result, gen_out, gen, want))
    for gen in GENS[:-1] + [2 ** 32 - 3]:
        for first_pn in (0, 1, 50, U64):
            for min_next in (U64, 0, 49, 50, 51, (1 << 62) - 1):
                for min_cur in (U64, 0, 49, 50, 51):
                    t = [[gen, first_pn]]
                    conns, res, pns, gens = [], [], [], []
                    if min_next != U64:
                        conns, res, pns, gens = conns + [0, 0], res + [1, 1], pns + [min_next, min_next + 5], gens + [gen + 1] * 2
                    if min_cur != U64:
                        conns, res, pns, gens = conns + [0, 0], res + [1, 1], pns + [min_cur + 3, min_cur], gens + [gen] * 2
                    upd = model.commit(t, conns, res, pns, gens)
                    lines.append("A %d %d %d %d %d %d %d\n" % (gen, first_pn, min_next, min_cur, t[0][0], t[0][1], int(upd == [0])))
    return lines


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("quic_phase") / "cases.txt"
    lines = _choice_lines() + _commit_lines()
    assert len(lines) > 15000
    with open(path, "w") as f:
        f.writelines(lines)
    return path, len(lines)


def _build(exe, extra):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC, *extra,
                    os.path.join(ROOT, "tests", "native", "quic_phase_check.cpp"), "-o", str(exe)], check=True)


@NEEDS
def test_quic_phase_rule_matches_the_model(cases, tmp_path):
    path, n = cases
    exe = tmp_path / "quic_phase_check"
    _build(exe, [])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(n)], r.stdout[-2000:] + r.stderr[-2000:]


@NEEDS
def test_quic_phase_rule_under_sanitizers(cases, tmp_path):
    """the same program with ASan + UBSan, run stand-alone (no preloaded runtime): it exits clean"""
    path, n = cases
    exe = tmp_path / "quic_phase_check_san"
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(n)], out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
