"""The parse arithmetic quic_parse_kernel.hip runs (hsig-picotls_amd/csrc/quic_parse.h), compiled for the host with plain g++
(no GPU) and run as a stand-alone program (tests/native/quic_parse_check.cpp) against the plain-Python reference
(tests/quic_parse_ref.py), over the datagrams of tests/quic_parse_cases.py, each walked under max_per_dgram 1, 3 and 16 and
with require_fixed_bit on and off:

  * every type under v1 and v2, version 0 and unknown versions; CID lengths 0, 1, 8, 20, 21, and 255 under an unknown version;
  * token lengths 0, 1, 63, 64 (the 1-to-2-byte varint boundary), 16383 and 16384, in the shortest and in wider encodings;
  * Length in all four varint widths, non-minimal ones included;
  * coalesced runs of 1 to 17 packets;
  * every truncation point of a long header: the datagram cut after each byte of the header in turn;
  * Length one below and one above what the datagram holds, Length 19 and 20;
  * the fixed bit clear; short headers around the pn_offset + 20 limit; random datagrams.

The connection-ID map (the hash, the probe loop, insert and the backward-shift removal that quic_parse.cpp runs on its
mirror and the kernel reads): at capacities 4 and 8 chains that start in the table's last slots and wrap around its end,
replace, removal from the head, the middle and the tail of a chain with a lookup of every survivor after each, and a
64K-entry map against a dict.

The same program is compiled a second time with -fsanitize=address,undefined and run over the same file as a plain
subprocess: every datagram and CID sits in an exactly-sized heap allocation, so an over-read of one byte stops it."""
import itertools
import os
import random
import shutil
import subprocess

import pytest

import quic_parse_cases as gen
import quic_parse_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "quic_parse_check.cpp")
INC = os.path.join(ROOT, "hsig-picotls_amd", "csrc")


def _hex(b):
    return bytes(b).hex() or "-"


def _walk_line(d, scl, mx, fixed):
    entries = ref.walk_datagram(d, scl, mx, fixed)
    nums = []
    for pos, w, more in entries:
        nums += [pos] + [w[f] for f in ref.WALK_FIELDS] + [int(more)]
    return "W %d %d %d %s %d %s\n" % (scl, mx, fixed, _hex(d), len(entries), " ".join(map(str, nums)))


def _chain(size, home, count, length=8):
    """`count` distinct CIDs whose home slot in a table of `size` entries is `home`"""
    out = []
    if count == 0:
        return out
    for k in itertools.count():
        cid = k.to_bytes(length, "big")
        if ref.cid_hash(cid) & (size - 1) == home:
            out.append(cid)
            if len(out) == count:
                return out


def _map_lines():
    rng = random.Random(77)
    lines = []

    def check(model, probes):
        lines.append("M size %d\n" % len(model))
        for cid in probes:
            lines.append("M get %s %d\n" % (_hex(cid), model.lookup(cid)))

    for capacity in (4, 8):
        size = 2 * capacity
        # chains from the table's last two slots: they wrap around its end; plus a neighbour chain at slot 0 and the empty CID
        for home, other in ((size - 1, 0), (size - 2, size - 1)):
            for victim_order in itertools.permutations(range(3)):  # remove head / middle / tail in every order
                model = ref.CidMap(capacity)
                lines.append("M new %d\n" % capacity)
                chain = _chain(size, home, 3) + _chain(size, other, capacity - 3 - 1) + [b""]
                absent = _chain(size, home, 5)[3:] + [bytes(20), b"\x00"]
                for k, cid in enumerate(chain):
                    model.set(cid, 100 + k)
                    lines.append("M set %s %d\n" % (_hex(cid), 100 + k))
                check(model, chain + absent)
                model.set(chain[1], 7)  # replace
                lines.append("M set %s 7\n" % _hex(chain[1]))
                check(model, chain + absent)
                for v in victim_order:
                    model.remove(chain[v])
                    lines.append("M del %s\n" % _hex(chain[v]))
                    lines.append("M del %s\n" % _hex(absent[0]))  # removing an absent CID changes nothing
                    check(model, chain + absent)
                model.set(chain[0], 9)  # and the freed slots take entries again
                lines.append("M set %s 9\n" % _hex(chain[0]))
                check(model, chain + absent)
    # 64K entries of every length against the dict, then half of them removed
    n = 1 << 16
    model = ref.CidMap(n)
    lines.append("M new %d\n" % n)
    cids = list({rng.randbytes(rng.choice((1, 4, 8, 8, 8, 16, 20))) for _ in range(n - 1)}) + [b""]
    for k, cid in enumerate(cids):
        model.set(cid, k)
        lines.append("M set %s %d\n" % (_hex(cid), k))
    check(model, cids[::7] + [rng.randbytes(8) for _ in range(2000)])
    for cid in cids[::2]:
        model.remove(cid)
        lines.append("M del %s\n" % _hex(cid))
    check(model, cids)
    return lines


def _write_cases(path):
    datagrams = walks = 0
    with open(path, "w") as f:
        for d, _ in gen.cases(seed=9000, random_fill=7000):
            datagrams += 1
            scls = (0, 8, 20)
            for k, (mx, fixed) in enumerate(itertools.product((1, 3, 16), (0, 1))):
                f.write(_walk_line(d, scls[(datagrams + k) % 3], mx, fixed))
                walks += 1
        lines = _map_lines()
        f.writelines(lines)
    return datagrams, walks + len(lines)


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("quic_parse") / "cases.txt"
    datagrams, lines = _write_cases(path)
    assert datagrams >= 10000
    return path, lines


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *extra, "-I", INC, SRC, "-o", str(exe)], check=True)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_quic_parse_functions_match_reference(case_file, tmp_path):
    path, lines = case_file
    exe = _build(tmp_path, "quic_parse_check", ["-O2"])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == f"ok {lines}", r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_quic_parse_functions_under_sanitizers(case_file, tmp_path):
    """the same program and cases under AddressSanitizer + UndefinedBehaviorSanitizer: no read past an exactly-sized datagram"""
    path, lines = case_file
    exe = _build(tmp_path, "quic_parse_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                     "-fno-omit-frame-pointer"])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == f"ok {lines}", r.stdout[-2000:] + r.stderr[-4000:]

