"""Received packet numbers tracked on the GPU (include/ptls_hip.h 2k; hsig-picotls_amd/csrc/quic_track_kernel.hip,
quic_rx.cpp).  Exact, no tolerance anywhere: every verdict, the whole state table, the whole expected-pn table and the list of
touched connections against the plain-Python model (tests/quic_track_ref.py).  The state table, the expected-pn table,
d_verdict and d_touched start sentinel-filled with 8 elements to spare, and what lies behind the elements a call owns must
come back untouched.  The cases are tests/quic_track_cases.py's, which tests/test_quic_track_ref.py and
tests/test_quic_track_native.py hold against the model and the host build of the same code.

Packets are real and small (20-byte payloads).  Where a case needs numbers that the wire cannot cheaply produce, the test opens
real packets and then overwrites its own d_result / d_pn_out with the case's values before the track call: they are the
caller's arrays.  There every fourth entry is followed by an entry that cannot be opened, so that selected positions and
entry indices differ and the type is read through d_sel.

Sizes: 130 connections; the packet passes at 1, 255, 256, 257 and 2 049 packets (their workgroup is 256 threads, the claim
pass takes four packets per thread); the touched list's compaction at 2 047 / 2 048 / 2 049 connections (QP_SCAN_SPAN = 2048)."""
import ctypes

import numpy as np
import pytest
import torch

import ptls_hip
import quic_phase_cases as kgen
import quic_ref
import quic_track_cases as gen
import quic_track_ref as model
from test_gpu_quic import ALGO_OF, FILL, SENTINEL, U64, dev, image, key_material, keysets, place, stream  # noqa: F401
from test_gpu_quic_keyphase import Keys, Opened as KpOpened, commit, keyed, lay_out as kp_lay_out, phase_table  # noqa: F401
from test_gpu_quic_parse import E2E_CIDS, NCONN, lay_out as dgram_lay_out
from test_gpu_quic_rx import ALL, SEL_SENT, i64, load

pytestmark = pytest.mark.gpu
ALGOS = ["aes128", "aes256", "chacha"]
VERDICT_SENT, TOUCHED_SENT, SPACE_SENT = 0xD7D7D7D7, 0xC9C9C9C9, 0xEEEEEEEEEEEEEEEE
PAYLOAD = stream("gpu-quic-track-payload", 20)
NEW, DUP, OLD, NONE = ptls_hip.QUIC_PN_NEW, ptls_hip.QUIC_PN_DUPLICATE, ptls_hip.QUIC_PN_TOO_OLD, ptls_hip.QUIC_PN_NONE
assert (NONE, NEW, DUP, OLD) == (model.NONE, model.NEW, model.DUPLICATE, model.TOO_OLD)


def u32(values):
    return torch.from_numpy(np.array(values, dtype=np.uint32).view(np.int32)).cuda()


def read_u32(t):
    return t.cpu().numpy().view(np.uint32)


def read_u64(t):
    return [int(x) & U64 for x in t.cpu().tolist()]


class State:
    """the caller's device arrays of a track call, sentinel-filled with 8 elements to spare: the state table, the expected-pn
    table (or none), d_verdict for m packets and d_touched"""

    def __init__(self, count, spaces, expected, m):
        self.count, self.m = count, m
        flat = [x for s in spaces for x in s] + [SPACE_SENT] * 16
        self.d_spaces = i64(flat)
        self.expected_len = len(expected) if expected is not None else 0
        self.d_expected = i64(list(expected) + [SENTINEL] * 8) if expected is not None else None
        self.d_verdict = u32(np.full(m + 8, VERDICT_SENT))
        self.d_touched = u32(np.full(count + 8, TOUCHED_SENT))

    def track(self, rx, d_sel, d_res, d_pn):
        self.n = rx.track(self.d_spaces, self.count, d_sel, d_res, d_pn, self.d_verdict, self.d_touched, self.d_expected,
                          self.expected_len)
        torch.cuda.synchronize()
        return self

    def spaces(self):
        flat = read_u64(self.d_spaces)
        assert flat[6 * self.count:] == [SPACE_SENT] * 16
        return [flat[2 * p: 2 * p + 2] for p in range(3 * self.count)]

    def expected(self):
        if self.d_expected is None:
            return None
        flat = read_u64(self.d_expected)
        assert flat[self.expected_len:] == [SENTINEL] * 8
        return flat[:self.expected_len]

    def verdicts(self, m=None):
        m = self.m if m is None else m
        v = read_u32(self.d_verdict)
        assert (v[m:] == VERDICT_SENT).all()
        return v[:m].tolist()

    def touched(self):
        t = read_u32(self.d_touched)
        assert self.n <= self.count and (t[self.n:] == TOUCHED_SENT).all()
        return t[:self.n].tolist()

    def check(self, want):
        verdicts, touched, after, exp = want
        got = self.verdicts()
        assert got == verdicts, next((j, g, w) for j, (g, w) in enumerate(zip(got, verdicts)) if g != w)
        assert self.spaces() == after and self.expected() == exp and self.touched() == touched


# ---- cases with the model's numbers: one real packet, opened under every connection's slot, then the case's values ----

PN = 0x1234
HEADER = b"\x41" + stream("gpu-quic-track-cid", 8) + PN.to_bytes(2, "big")


class OneKey:
    """keysets whose every slot holds one key: the one packet opens as any connection's"""

    def __init__(self, engine, algo, nslots):
        kind, ksz = ALGO_OF[algo]
        key, iv, hp = stream("gpu-quic-track-key-" + algo, ksz), stream("gpu-quic-track-iv-" + algo, 12), stream("gpu-quic-track-hp-" + algo, ksz)
        self.nslots = nslots
        self.ks, self.hp = ptls_hip.KeySet(engine, ksz, nslots, algo=kind), ptls_hip.KeySet(engine, ksz, nslots, algo=kind)
        self.ks.set(0, key * nslots, iv * nslots)
        self.hp.set(0, hp * nslots, None)
        self.packet = quic_ref.protect(algo, key, iv, hp, HEADER, PN, PAYLOAD)


@pytest.fixture(scope="module")
def onekey(engine):
    made = {}

    def get(algo, nslots=132):
        if (algo, nslots) not in made:
            made[algo, nslots] = OneKey(engine, algo, nslots)
        return made[algo, nslots]

    yield get
    torch.cuda.synchronize()
    for k in made.values():
        k.ks.close()
        k.hp.close()


class Synthetic:
    """a Call's packets as real packets in a receive object, opened: d_sel as the open call left it, d_result and d_pn_out
    overwritten with the call's values.  rx: an existing receive object to load them into (the caller closes it)"""

    def __init__(self, engine, keys, call, duds=True, rx=None):
        self.call, self.m = call, len(call.packets)
        entries = []
        for j in range(self.m):
            entries.append(j)
            if duds and j % 4 == 1:
                entries.append(None)  # an entry that cannot be opened: the positions behind it are not their entry indices
        n = len(entries)
        raw = keys.packet
        offs, total = place([len(raw)] * n)
        out_offs, out_total = place([24] * n)
        pkts, info = np.zeros(n, dtype=ptls_hip.QUIC_PACKET_DTYPE), np.zeros(n, dtype=ptls_hip.QUIC_PKTINFO_DTYPE)
        pkts["pkt_off"], pkts["data_off"], pkts["pn"], pkts["pkt_len"] = offs, out_offs, PN - 3, len(raw)
        pkts["pn_offset"] = [9 if e is not None else 0 for e in entries]
        pkts["key"] = pkts["hp_key"] = info["conn"] = [call.packets[e][0] if e is not None else 0 for e in entries]
        # (a dud carries a type of another space than the packet in front of it: a type read at the position shows)
        info["type"] = [call.packets[e][1] if e is not None else (model.INITIAL if call.packets[entries[k - 1]][1] != model.INITIAL
                                                                   else model.ONE_RTT) for k, e in enumerate(entries)]
        self.own_rx = rx is None
        self.rx = ptls_hip.QuicRx(engine, 0, n) if rx is None else rx
        try:
            load(self.rx, pkts, info)
            cap = n + 8
            d_out = torch.full((out_total,), FILL, dtype=torch.uint8, device="cuda")
            self.d_sel = u32(np.full(cap, SEL_SENT))
            self.d_res = torch.full((cap,), SENTINEL, dtype=torch.int64, device="cuda")
            self.d_pn = torch.full((cap,), SENTINEL, dtype=torch.int64, device="cuda")
            rep = self.rx.open(keys.ks, keys.hp, dev(image(total, offs, [raw] * n)), total, d_out, out_total, self.d_sel, self.d_res,
                               self.d_pn)
            torch.cuda.synchronize()
            m = self.m
            assert rep.n_selected == m and read_u32(self.d_sel)[:m].tolist() == [k for k, e in enumerate(entries) if e is not None]
            assert read_u64(self.d_res)[:m] == [len(PAYLOAD)] * m and read_u64(self.d_pn)[:m] == [PN] * m  # real packets, really opened
            _, _, results, pns = call.columns()
            self.d_res[:m] = i64(results)
            self.d_pn[:m] = i64(pns)
        except BaseException:
            self.close()
            raise

    def run(self, expected="zeros", spaces=None, count=None):
        """one track call from the call's states (or `spaces`) with fresh arrays, checked against the model"""
        call = self.call if count is None else gen.Call(count, self.call.spaces[:3 * count], self.call.packets,
                                                        min(self.call.expected_len, 3 * count))
        if expected == "zeros":
            expected = [0] * call.expected_len
        st = State(call.count, call.spaces if spaces is None else spaces, expected, self.m).track(self.rx, self.d_sel, self.d_res, self.d_pn)
        st.check(call.want(expected, spaces=spaces))
        return st

    def close(self):
        torch.cuda.synchronize()
        if self.own_rx:
            self.rx.close()


@pytest.fixture
def synthetic(engine):
    made = []

    def make(keys, call, **kw):
        made.append(Synthetic(engine, keys, call, **kw))
        return made[-1]

    yield make
    for s in made:
        s.close()


@pytest.mark.parametrize("algo,part", list(zip(ALGOS, range(3))))
def test_the_case_list(synthetic, onekey, algo, part):
    """a third of the grid per cipher over the 390 spaces of 130 connections: untouched spaces come back byte-identical (the
    whole table is compared), only touched elements below expected_count are written; first with a smaller table (the object's
    scratch grows between the calls), then without an expected-pn table, then the replay of the whole call"""
    call = gen.case_list(part)
    s = synthetic(onekey(algo), call)
    assert len(call.packets) > 600 and call.expected_len < 3 * call.count
    s.run(count=60)
    st = s.run()
    assert set(st.verdicts()) == {NONE, NEW, DUP, OLD} and st.n > 60
    assert st.expected() != [0] * call.expected_len
    s.run(expected=None)
    again = s.run(spaces=st.spaces())
    assert NEW not in again.verdicts() and again.n == 0 and again.spaces() == st.spaces()


def track_slots(m):
    """positions of the candidate table of m selected packets (csrc/quic_track.h quic_track_slots): the power of two from 2 m, at least 2"""
    size = 2
    while size < 2 * m:
        size *= 2
    return size


def test_the_candidate_table_grows(engine, synthetic, onekey):
    """one receive object: 3 packets of 2 connections loaded, opened and tracked, then 200 packets of 5 connections.  Between
    the calls the candidate table grows (8 positions, then 512) and so do the per-space accumulators and the scan levels
    (count 2, then 5): verdicts, the whole state table, the expected-pn table and the touched list are the model's both times,
    so the regrown accumulators were zero and the regrown table held no candidate of the first call"""
    small, large = gen.distinct_call(3, count=2), gen.distinct_call(200, count=5)
    assert (track_slots(3), track_slots(200)) == (8, 512) and large.count > small.count
    rx = ptls_hip.QuicRx(engine, 0, 256)
    try:
        a = synthetic(onekey("aes128"), small, rx=rx).run()
        assert a.verdicts() == [NEW] * 3 and a.touched() == [0, 1]
        b = synthetic(onekey("aes128"), large, rx=rx).run()
        assert b.verdicts() == [NEW] * 200 and b.touched() == [0, 1, 2, 3, 4]
    finally:
        torch.cuda.synchronize()
        rx.close()


def test_order(synthetic, onekey):
    """the same packets loaded in a permuted entry order: the state, the expected table and the touched list are identical, the
    verdicts are the model's for that order"""
    call = gen.case_list(1)
    a = synthetic(onekey("aes128"), call).run()
    for seed in (1, 2):
        b = synthetic(onekey("aes128"), call.permuted(seed)).run()
        assert b.spaces() == a.spaces() and b.expected() == a.expected() and b.touched() == a.touched()
        assert b.verdicts() != a.verdicts() and sorted(b.verdicts()) == sorted(a.verdicts())


def test_bulk_traffic_of_one_connection(synthetic, onekey):
    """4 096 packets in buffer order, all but the 44 failed ones new, laid out so that the claim pass folds a lane's successive
    packets, flushes when the space changes, reduces waves that hold one space (with the largest number in lane 37, and with
    lanes that hold nothing) and meets waves that hold two spaces: the window is all ones and next is right"""
    call = gen.bulk_call()
    paths = gen.claim_paths(call)
    assert paths["fold"] > 2500 and paths["flush"] >= 100 and paths["reduce"] >= 12 and paths["partial"] >= 1 and paths["split"] >= 2
    assert 37 in paths["top_lanes"]
    st = synthetic(onekey("aes128"), call, duds=False).run()
    v = st.verdicts()
    assert v.count(NEW) == 4096 - 44 and v.count(NONE) == 44
    n2 = sum(1 for p in call.packets if p[:2] == (0, model.ONE_RTT) and p[2] != U64)
    assert st.spaces()[2] == [1000 + n2, (1 << 64) - 1] and st.touched() == [0, 1]


@pytest.mark.parametrize("m", [1, 255, 256, 257, 2049])
def test_the_table_with_distinct_packets(synthetic, onekey, m):
    st = synthetic(onekey("chacha"), gen.distinct_call(m)).run()
    assert st.verdicts() == [NEW] * m


def test_the_table_with_copies(synthetic, onekey):
    """257 copies of one packet: position 0 is new, the 256 others are its duplicates; triples whose copies sit in different
    workgroups: the lowest position of each is new"""
    st = synthetic(onekey("aes128"), gen.copies_call(257)).run()
    assert st.verdicts() == [NEW] + [DUP] * 256 and st.spaces()[5] == [96, 1 | 1 << 6]
    call = gen.triples_call()
    assert len(gen.spread_triples(call)) > 100
    v = synthetic(onekey("aes128"), call).run().verdicts()
    assert v[:900] == [NEW] * 300 + [DUP] * 600 and v[900:] == [NEW] * (2049 - 900)


@pytest.mark.parametrize("count", [2047, 2048, 2049])
def test_touched_compaction_seam(synthetic, onekey, count):
    call = gen.seam_call(count)
    st = synthetic(onekey("chacha", 2056), call).run()
    assert count - 1 in st.touched() and 400 < st.n < 450
    # a smaller table than the packets' connections: those outside are left alone
    synthetic(onekey("chacha", 2056), call).run(count=100)


# ---- the loop closed: parse, open, track, parse again, with numbers on the wire ----

def wire_packet(algo, conn, pn, pn_len, forged=False):
    keys, ivs, hps = key_material(algo)
    header = bytes([0x40 | (pn_len - 1)]) + E2E_CIDS[conn] + (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big")
    pkt = bytearray(quic_ref.protect(algo, keys[conn], ivs[conn], hps[conn], header, pn, PAYLOAD))
    if forged:
        pkt[-1] ^= 0x10  # a tag bit: the header, and with it the packet number, reads as sent
    return bytes(pkt)


class Loop:
    """12 connections' 1-RTT space: the device's state and expected-pn tables, and the model's beside them"""

    def __init__(self, engine, keysets, algo):
        self.engine, self.algo = engine, algo
        self.ks, self.hp = keysets(algo)
        self.spaces = [[0, 0] for _ in range(3 * NCONN)]
        self.expected = [0] * (3 * NCONN)
        self.d_spaces = i64([0] * (6 * NCONN) + [SPACE_SENT] * 16)
        self.d_expected = i64(self.expected + [SENTINEL] * 8)
        self.map = ptls_hip.QuicCidMap(engine, NCONN)
        self.map.set(E2E_CIDS, list(range(NCONN)))

    def close(self):
        torch.cuda.synchronize()
        self.map.close()

    def datagrams(self, sent, seed=5):
        """sent: (conn, pn, pn_len, forged) per datagram"""
        return dgram_lay_out([(wire_packet(self.algo, *s), b"") for s in sent], seed)

    def open(self, buf, dg, d_expected):
        """parse with the table d_expected and open: (rx, results, packet numbers, d_sel, d_res, d_pn)"""
        rx = ptls_hip.QuicRx(self.engine, len(dg), len(dg))
        try:
            d_buf, total = dev(buf), len(buf)
            n = rx.parse(dg, d_buf, total, cidmap=self.map, short_cid_len=8, expected_pn=d_expected, expected_count=3 * NCONN)
            assert n == len(dg)
            d_out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
            d_sel = u32(np.full(n + 8, SEL_SENT))
            d_res = torch.full((n + 8,), SENTINEL, dtype=torch.int64, device="cuda")
            d_pn = torch.full((n + 8,), SENTINEL, dtype=torch.int64, device="cuda")
            rep = rx.open(self.ks, self.hp, d_buf, total, d_out, total, d_sel, d_res, d_pn, type_mask=1 << model.ONE_RTT)
            torch.cuda.synchronize()
            assert rep.n_selected == n
            return rx, read_u64(d_res)[:n], read_u64(d_pn)[:n], d_sel, d_res, d_pn
        except BaseException:
            torch.cuda.synchronize()
            rx.close()
            raise

    def step(self, sent):
        """parse with the device's table, open, track: (results, packet numbers, verdicts, touched); the device's tables are
        compared whole with the model's"""
        buf, dg = self.datagrams(sent)
        rx, res, pns, d_sel, d_res, d_pn = self.open(buf, dg, self.d_expected)
        try:
            m = len(sent)
            d_verdict, d_touched = u32(np.full(m + 8, VERDICT_SENT)), u32(np.full(NCONN + 8, TOUCHED_SENT))
            n = rx.track(self.d_spaces, NCONN, d_sel, d_res, d_pn, d_verdict, d_touched, self.d_expected, 3 * NCONN)
            torch.cuda.synchronize()
            want_v, want_t = model.track(self.spaces, self.expected, NCONN, [s[0] for s in sent], [model.ONE_RTT] * m, res, pns)
            v, t = read_u32(d_verdict), read_u32(d_touched)
            assert (v[m:] == VERDICT_SENT).all() and (t[n:] == TOUCHED_SENT).all()
            assert v[:m].tolist() == want_v and t[:n].tolist() == want_t
            assert read_u64(self.d_spaces) == [x for s in self.spaces for x in s] + [SPACE_SENT] * 16
            assert read_u64(self.d_expected) == self.expected + [SENTINEL] * 8
            return res, pns, want_v, want_t
        finally:
            torch.cuda.synchronize()
            rx.close()


@pytest.fixture
def loop(engine, keysets):
    made = []

    def make(algo):
        made.append(Loop(engine, keysets, algo))
        return made[-1]

    yield make
    for lp in made:
        lp.close()


STEP1 = [(c, pn, 2, False) for c in range(NCONN) for pn in (0, 500 + c, 990 + c % 5, 1000)]
STEP2 = [(c, pn, 1, False) for pn in (1001, 1003, 1002) for c in range(NCONN)]


@pytest.mark.parametrize("algo", ["aes128", "chacha"])
def test_the_gap_and_the_loop_closed(loop, algo):
    """2-byte packet numbers up to 1 000 parsed with a zero table, opened and tracked; then 1-byte numbers from 1 001: parsed
    with the table as it was before the track call, every one decodes wrongly and fails authentication (the behaviour without
    rx_track); parsed with the table the device left, every one opens and is new.  Then the same datagrams again: every one is a
    duplicate, no state byte changes, nothing is touched"""
    lp = loop(algo)
    before = i64([0] * (3 * NCONN))
    res, pns, v, t = lp.step(STEP1)
    assert res == [20] * len(STEP1) and pns == [s[1] for s in STEP1] and v == [NEW] * len(STEP1) and t == list(range(NCONN))
    assert lp.expected == [0, 0, 1001] * NCONN and lp.spaces[2] == [1001, 1 | 1 << 10]
    buf, dg = lp.datagrams(STEP2)
    rx, res, pns, *_ = lp.open(buf, dg, before)
    rx.close()
    assert res == [U64] * len(STEP2) and all(pn != s[1] and pn < 256 for pn, s in zip(pns, STEP2))
    res, pns, v, t = lp.step(STEP2)
    assert res == [20] * len(STEP2) and pns == [s[1] for s in STEP2] and v == [NEW] * len(STEP2) and t == list(range(NCONN))
    assert lp.expected == [0, 0, 1004] * NCONN and lp.spaces[2] == [1004, 0b1111 | 1 << 13]
    # the replay
    state = [list(s) for s in lp.spaces]
    res, pns, v, t = lp.step(STEP2)
    assert res == [20] * len(STEP2) and v == [DUP] * len(STEP2) and t == [] and lp.spaces == state


@pytest.mark.parametrize("algo", ["aes128", "chacha"])
def test_forged_advance(loop, algo):
    """packets with a flipped tag bit and the highest numbers of the call: no verdict, the state is as without them, and the
    next parse still decodes"""
    lp = loop(algo)
    lp.step(STEP1)
    sent = [(c, 1001 + k, 1, False) for c in range(NCONN) for k in range(2)] + [(c, 1100 + c, 1, True) for c in range(NCONN)]
    res, pns, v, t = lp.step(sent)
    assert res == [20] * (2 * NCONN) + [U64] * NCONN and pns == [s[1] for s in sent]  # the forged numbers did decode
    assert v == [NEW] * (2 * NCONN) + [NONE] * NCONN and lp.expected == [0, 0, 1003] * NCONN
    follow = [(c, 1003, 1, False) for c in range(NCONN)]
    res, pns, v, t = lp.step(follow)
    assert res == [20] * NCONN and pns == [1003] * NCONN and v == [NEW] * NCONN


# ---- beside the key phase ----

@pytest.mark.parametrize("algo", ["aes128", "chacha"])
def test_with_the_key_phase(engine, keyed, algo):
    """rx_open_keyphase, then track and commit in both orders: identical outcomes; previous-generation packets are tracked in
    space 2 like any other 1-RTT packet"""
    case = kgen.three_banks(algo)
    keys = keyed(case)
    buf, pkts, pkt_total, out_total = kp_lay_out(case)
    info = np.zeros(len(pkts), dtype=ptls_hip.QUIC_PKTINFO_DTYPE)
    info["type"] = [model.HANDSHAKE if p.long else model.ONE_RTT for p in case.packets]
    info["conn"] = pkts["key"]
    spaces = [[kgen.MID + 3, 0b101] if p % 3 == 2 and p % 2 else [0, 0] for p in range(3 * case.count)]
    outcomes = []
    for track_first in (True, False):
        rx = ptls_hip.QuicRx(engine, 0, len(pkts))
        try:
            load(rx, pkts, info)
            d_phase = dev(phase_table(case.states).view(np.uint8))
            o = KpOpened(rx, keys, d_phase, case.count, case.stride, dev(buf), pkt_total, out_total)
            assert o.sel == list(range(len(pkts)))
            d_sel = u32(o.sel + [SEL_SENT] * 8)
            st = State(case.count, spaces, [7] * (3 * case.count), o.m)
            if track_first:
                st.track(rx, d_sel, o.d_res, o.d_pn)
                upd, table = commit(rx, o, d_phase, case.count)
            else:
                upd, table = commit(rx, o, d_phase, case.count)
                st.track(rx, d_sel, o.d_res, o.d_pn)
            call = gen.Call(case.count, spaces, [(p.conn, int(t), r, pn) for p, t, r, pn in zip(case.packets, info["type"], o.res, o.pns)])
            st.check(call.want([7] * (3 * case.count)))
            outcomes.append((st.verdicts(), st.spaces(), st.expected(), st.touched(), upd, table))
        finally:
            torch.cuda.synchronize()
            rx.close()
    assert outcomes[0] == outcomes[1] and len(outcomes[0][4]) > 20
    previous = [j for j, p in enumerate(case.packets) if p.want_gen == case.states[p.conn][0] - 1 and o.res[j] != U64]
    assert len(previous) > 20 and all(outcomes[0][0][j] != NONE for j in previous) and {NEW, OLD} <= set(outcomes[0][0])


# ---- refusals ----

def test_refusals_and_nothing_selected(engine, onekey):
    """every refusal of rx_track with a real receive object: nothing launched, nothing written; a call behind an open that
    selected nothing returns 0 and writes nothing"""
    keys = onekey("aes128")
    call = gen.distinct_call(40)
    L = ptls_hip.lib()
    s = Synthetic(engine, keys, call)
    try:
        st = State(call.count, call.spaces, [0] * (3 * call.count), s.m)
        n = ctypes.c_size_t(77)
        P = ptls_hip._ptr

        def track(obj=s.rx.ptr, spaces=st.d_spaces, count=call.count, exp=st.d_expected, exp_n=3 * call.count, verdict=st.d_verdict,
                  touched=st.d_touched, null_tr=False, sel=s.d_sel, res=s.d_res, pn=s.d_pn, n_touched=n):
            tr = ptls_hip.QuicRxTrack(P(spaces), count, P(exp), exp_n, P(verdict), P(touched))
            return L.ptls_hip_quic_rx_track(obj, None if null_tr else ctypes.addressof(tr), P(sel), P(res), P(pn),
                                            ctypes.byref(n_touched) if n_touched is not None else None, None)

        def untouched():
            torch.cuda.synchronize()
            assert n.value == 77 and st.verdicts(0) == [] and (read_u32(st.d_touched) == TOUCHED_SENT).all()
            assert st.spaces() == call.spaces and st.expected() == [0] * (3 * call.count)

        refusals = [(dict(obj=None), "null receive object"), (dict(null_tr=True), "null receive object, parameters"),
                    (dict(sel=None), "array or n_touched"), (dict(res=None), "array or n_touched"), (dict(pn=None), "array or n_touched"),
                    (dict(n_touched=None), "array or n_touched"), (dict(spaces=None), "null state, verdict or touched array"),
                    (dict(verdict=None), "null state, verdict or touched array"), (dict(touched=None), "null state, verdict or touched array"),
                    (dict(count=0), "a connection count of 0 is outside 1 .. 2^32 - 1"),
                    (dict(count=1 << 32), "a connection count of 4294967296 is outside"),
                    (dict(exp=None), "no expected-pn table, but %d entries of it" % (3 * call.count))]
        for kw, msg in refusals:
            assert track(**kw) == ptls_hip.EINVAL, kw
            assert "quic_rx_track:" in ptls_hip.last_error() and msg in ptls_hip.last_error(), (kw, ptls_hip.last_error())
        untouched()
        # entries loaded again: the open call in front is gone
        d_pkts = dev(s.rx.packets().view(np.uint8))
        d_info = dev(s.rx.info().view(np.uint8))
        n_entries = len(s.rx)
        s.rx.set_packets(d_pkts, d_info, n_entries)
        assert track() == ptls_hip.EINVAL and "no open call on the object since its entries were loaded" in ptls_hip.last_error()
        # ... without info records: no packet-number space is known
        s.rx.set_packets(d_pkts, None, n_entries)
        total = int(d_pkts.cpu().numpy().view(ptls_hip.QUIC_PACKET_DTYPE)["pkt_off"].max()) + 256
        d_buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        d_out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        d_sel, d_res, d_pn = u32(np.full(n_entries + 8, SEL_SENT)), i64([SENTINEL] * (n_entries + 8)), i64([SENTINEL] * (n_entries + 8))
        rep = s.rx.open(keys.ks, keys.hp, d_buf, total, d_out, total, d_sel, d_res, d_pn)
        assert rep.n_selected == s.m
        assert track(sel=d_sel, res=d_res, pn=d_pn) == ptls_hip.EINVAL and "loaded without info records" in ptls_hip.last_error()
        untouched()
        # nothing selected: 0, *n_touched = 0, nothing written
        s.rx.set_packets(d_pkts, d_info, n_entries)
        rep = s.rx.open(keys.ks, keys.hp, d_buf, total, d_out, total, d_sel, d_res, d_pn, type_mask=1 << model.RETRY)
        assert rep.n_selected == 0
        assert track() == 0 and n.value == 0
        n.value = 77
        untouched()
    finally:
        s.close()
