"""ACK frames written on the GPU from the tracked packet numbers (include/ptls_hip.h 2m;
hsig-picotls_amd/csrc/quic_ack_kernel.hip, quic_rx.cpp).  Exact, no tolerance anywhere: every status, offset and length, the
whole frame buffer, the whole request array and the whole (untouched) state table against the plain-Python model
(tests/quic_ack_ref.py).  Every array starts sentinel-filled with spare elements, the frame buffer 0xA5-filled with 64 spare
bytes, and everything is compared whole.  The cases are tests/quic_ack_cases.py's, which tests/test_quic_ack_ref.py and
tests/test_quic_ack_native.py hold against hand-written byte strings and the host build of the same code.

Sizes: 130 connections; lists of 1, 63 / 64 / 65 (a wave), 255 / 256 / 257 (the passes' workgroup) and 2 047 / 2 048 / 2 049
entries (QP_SCAN_SPAN = 2048).  A frame's delay is the call's, so a 5-byte frame (1-byte delay) and an 81-byte frame (8-byte
delay) cannot lie in one call: the neighbours across a workgroup edge are 5 / 74 bytes with ack_delay 0 and 12 / 81 with
2^62 - 1."""
import ctypes

import numpy as np
import pytest
import torch

import ptls_hip
import quic_ack_cases as gen
import quic_ack_ref as model
import quic_tx_cases as tgen
from quic_tx_ref import Conn
from test_gpu_quic import FILL, SENTINEL, U64, dev
from test_gpu_quic_tx import LOOP_CIDS, LOOP_CONNS, Sealed, TxKeys, conn_table, phase_table

pytestmark = pytest.mark.gpu
STATUS_SENT, OFF_SENT, LEN_SENT, SEL_SENT, GEN_SENT, VERDICT_SENT, TOUCHED_SENT = (0xD1D1D1D1, 0xB8B8B8B8, 0xC7C7C7C7, 0xC3C3C3C3, 0xB4B4B4B4,
                                                                               0xD7D7D7D7, 0xC9C9C9C9)
SPACE_SENT, REQ_FILL, SPARE = 0xEEEEEEEEEEEEEEEE, 0xE1, 64
REQ = ptls_hip.QUIC_TXREQ_DTYPE
OK = ptls_hip.QUIC_ACK_OK
assert (OK, ptls_hip.QUIC_ACK_NO_CONN, ptls_hip.QUIC_ACK_EMPTY, ptls_hip.QUIC_ACK_STATE) == (model.OK, model.NO_CONN, model.EMPTY, model.STATE)
assert ptls_hip.QUIC_ACK_MAX == model.ACK_MAX


def u32(values):
    return torch.from_numpy(np.array(values, dtype=np.uint32).view(np.int32)).cuda()


def i64(values):
    return torch.tensor(np.array(values, dtype=np.uint64).view(np.int64), device="cuda")


def read_u32(t):
    return t.cpu().numpy().view(np.uint32)


def read_u64(t):
    return [int(x) & U64 for x in t.cpu().tolist()]


def req_rows(reqs):
    a = np.zeros(len(reqs), dtype=REQ)
    for f, k in (("data_off", 0), ("pkt_off", 1), ("conn", 2), ("len", 3)):
        a[f] = np.array([r[k] for r in reqs], dtype=REQ[f])
    return a


class Arrays:
    """the caller's device arrays of an ack call, sentinel-filled with spare elements: the state table, the list, the frame
    buffer (81 bytes per entry and SPARE more), the three per-entry arrays and the request array"""

    def __init__(self, call):
        self.call, self.n = call, len(call.conns)
        n = self.n
        self.flat = [x for s in call.spaces for x in s] + [SPACE_SENT] * 16
        self.d_spaces = i64(self.flat)
        self.d_list = u32(call.conns + [TOUCHED_SENT] * 4)
        self.frames_len = model.ACK_MAX * n
        self.d_frames = torch.full((self.frames_len + SPARE,), FILL, dtype=torch.uint8, device="cuda")
        self.d_status, self.d_off, self.d_len = u32(np.full(n + 8, STATUS_SENT)), u32(np.full(n + 8, OFF_SENT)), u32(np.full(n + 8, LEN_SENT))
        self.d_reqs = torch.full(((n + 4) * REQ.itemsize,), REQ_FILL, dtype=torch.uint8, device="cuda")

    def run(self, rx):
        c = self.call
        self.rep = rx.ack(self.d_spaces, c.count, c.space, self.d_list, self.n, self.d_frames, self.frames_len, self.d_status, self.d_off,
                          self.d_len, self.d_reqs, ack_delay=c.ack_delay, max_ranges=c.max_ranges, in_off=c.in_off, pkt_base=c.pkt_base,
                          pkt_stride=c.pkt_stride)
        torch.cuda.synchronize()
        return self

    def read(self):
        self.status, self.off, self.len = read_u32(self.d_status), read_u32(self.d_off), read_u32(self.d_len)
        self.frames = self.d_frames.cpu().numpy()
        self.reqs = self.d_reqs.cpu().numpy()
        return self

    def untouched(self):
        """a refused call, or one with nothing to write: every array as it was"""
        self.read()
        assert (self.status == STATUS_SENT).all() and (self.off == OFF_SENT).all() and (self.len == LEN_SENT).all()
        assert (self.frames == FILL).all() and (self.reqs == REQ_FILL).all() and read_u64(self.d_spaces) == self.flat

    def check(self, want=None):
        """everything, whole, against the model's outcome"""
        o = self.call.want() if want is None else want
        self.read()
        n = self.n
        assert (self.status[n:] == STATUS_SENT).all() and (self.off[n:] == OFF_SENT).all() and (self.len[n:] == LEN_SENT).all()
        got = self.status[:n].tolist()
        assert got == o.status, next((j, g, w) for j, (g, w) in enumerate(zip(got, o.status)) if g != w)
        assert self.len[:n].tolist() == o.frame_len and self.off[:n].tolist() == o.frame_off
        assert (self.rep.n_frames, self.rep.bytes) == (len(o.reqs), len(o.bytes))
        want_frames = np.full(self.frames_len + SPARE, FILL, np.uint8)
        want_frames[:len(o.bytes)] = np.frombuffer(o.bytes, np.uint8)
        bad = np.flatnonzero(self.frames != want_frames)
        assert bad.size == 0, (int(bad[0]), int(self.frames[bad[0]]), int(want_frames[bad[0]]))
        want_reqs = np.full((n + 4) * REQ.itemsize, REQ_FILL, np.uint8)
        want_reqs[:len(o.reqs) * REQ.itemsize] = req_rows(o.reqs).view(np.uint8)
        assert np.array_equal(self.reqs, want_reqs)
        assert read_u64(self.d_spaces) == self.flat  # the state table is read, never written
        self.want = o
        return self


@pytest.fixture
def receiver(engine):
    made = []

    def make(max_dgrams=0, cap=1):
        made.append(ptls_hip.QuicRx(engine, max_dgrams, cap))
        return made[-1]

    yield make
    torch.cuda.synchronize()
    for rx in made:
        rx.close()


# ---- the shared cases ----

@pytest.mark.parametrize("space", [0, 1, 2])
def test_the_case_list(receiver, space):
    """every shape of entry over the 390 spaces of 130 connections, the list in no ascending order with duplicates and
    connections outside the table; the delay and the largest at every varint length, max_ranges at 0, 1, 30, 31, 32 and 2^32 - 1;
    in_off and the packet placement up to where 2^64 would wrap"""
    rx = receiver()
    seen, lengths = set(), set()
    top = (1 << 64) - 1
    for k, delay in enumerate(gen.DELAYS):
        keep = gen.MAX_RANGES[(k + space) % len(gen.MAX_RANGES)]
        call = gen.case_list(space, ack_delay=delay, max_ranges=keep, in_off=(k % 2) * (top - 81 * 147), pkt_base=(1 << 40) * k + 3,
                             pkt_stride=(1 << 55) if k % 3 == 0 else 1350)
        assert len(call.conns) == 147
        a = Arrays(call).run(rx).check()
        seen |= set(a.want.status)
        lengths |= set(a.want.frame_len)
    # (the inputs: every status, the shortest frame and long ones; the 81-byte frame is test_short_and_long_frames_...'s)
    assert seen == {model.OK, model.NO_CONN, model.EMPTY, model.STATE} and {0, 5} <= lengths and max(lengths) >= 70


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049])
def test_list_sizes(receiver, n):
    a = Arrays(gen.sized_call(n, ack_delay=n, pkt_base=1, pkt_stride=100)).run(receiver()).check()
    assert a.rep.n_frames <= n and (n < 63 or 0 < a.want.status.count(model.NO_CONN) < n // 8)
    assert n < 63 or {model.OK, model.EMPTY, model.STATE} <= set(a.want.status)


def test_duplicates_and_the_table_end(receiver):
    """the same connection listed five times gets five frames; count - 1 is the last connection, count and 2^32 - 1 are none"""
    count = 6
    spaces = [[100 + p, 0b1101 | p << 8] for p in range(3 * count)]
    call = gen.Call(count, spaces, 1, [5, 2, 5, 6, 5, 0xFFFFFFFF, 5, 5, 0, 6], ack_delay=9, in_off=1000, pkt_base=50, pkt_stride=90)
    a = Arrays(call).run(receiver()).check()
    no = model.NO_CONN
    assert a.want.status == [OK, OK, OK, no, OK, no, OK, OK, OK, no] and a.rep.n_frames == 7
    assert len({a.want.frames[j] for j in (0, 2, 4, 6, 7)}) == 1 and [r[2] for r in a.want.reqs] == [5, 2, 5, 5, 5, 5, 0]


def test_nothing_but_empty_spaces(receiver):
    """every listed space is empty: the three per-entry arrays are written (ACK_EMPTY, offset 0, length 0), and nothing else"""
    call = gen.empty_call()
    a = Arrays(call).run(receiver()).check()
    assert a.want.status == [model.EMPTY] * 300 and (a.rep.n_frames, a.rep.bytes) == (0, 0)
    assert (a.frames == FILL).all() and (a.reqs == REQ_FILL).all() and a.off[:300].tolist() == [0] * 300


@pytest.mark.parametrize("delay,lengths", [(0, [5, 74]), ((1 << 62) - 1, [12, 81])])
def test_short_and_long_frames_across_workgroup_edges(receiver, delay, lengths):
    a = Arrays(gen.edge_call(delay)).run(receiver()).check()
    assert a.want.frame_len[254:258] == lengths * 2 and a.want.frame_len[510:514] == lengths * 2 and a.rep.n_frames == 520


def test_the_scratch_grows(receiver):
    """one receive object: 5 entries, then 3 000 (the scan levels gain a level and are allocated anew), then 5 again in the
    larger scratch"""
    rx = receiver()
    for n in (5, 3000, 5):
        Arrays(gen.sized_call(n, seed=9, pkt_stride=7)).run(rx).check()


def test_a_permuted_list_gives_the_permuted_frames(receiver):
    rx = receiver()
    call = gen.case_list(2, ack_delay=70, pkt_stride=200)
    a = Arrays(call).run(rx).check()
    for seed in (1, 2):
        p = call.permuted(seed)
        b = Arrays(p).run(rx).check()
        assert p.conns != call.conns and sorted(b.want.frames) == sorted(a.want.frames) and b.rep.bytes == a.rep.bytes
        by_conn = {c: f for c, f in zip(call.conns, a.want.frames)}
        got = [b.frames[o: o + k].tobytes() for o, k in zip(b.off[:b.n].tolist(), b.len[:b.n].tolist())]
        assert got == [by_conn[c] for c in p.conns]


# ---- the loop closed: A's packets tracked at B, B's ACK frames sealed from the requests as they came out, read at A ----

@pytest.mark.parametrize("algo", ["aes128", "chacha"])
def test_the_loop_closed(engine, receiver, algo):
    """A sends 310 1-RTT packets through tx_seal; the network drops every fifth and all of connection 7 and replays two.  B runs
    rx_parse, rx_open_keyphase and rx_track, then rx_ack over d_touched and tx_seal over the requests as they came out.  A runs
    rx_parse and rx_open: its plaintexts are the frames, and the decoder reads from them exactly the packet numbers that B
    judged new and that lie within 64 of the connection's largest (connection 0 sent 90: its oldest lie further back)"""
    keys = TxKeys(engine, algo, LOOP_CONNS, LOOP_CONNS)
    made = []
    try:
        gens = [c % 3 for c in range(LOOP_CONNS)]
        a_conns = [Conn(next_pn=3 + c, gen=gens[c], dcid=LOOP_CIDS[c], flags=c & 1) for c in range(LOOP_CONNS)]
        items = [(0, 20)] * 90
        for c in range(1, LOOP_CONNS):
            items += [(c, 20 + c)] * 20
        reqs, in_len, buf_len = tgen.lay_out(items)
        call = tgen.Call(a_conns, reqs, in_len, buf_len, stride=LOOP_CONNS, hp_slots=LOOP_CONNS)
        made.append(ptls_hip.QuicTx(engine, len(reqs)))
        a = Sealed(engine, made[-1], keys, call, model_every=1 if algo != "chacha" else 32)
        assert a.status == [ptls_hip.QUIC_TX_SENT] * len(reqs)
        # the network
        deliver = [k for k in range(len(reqs)) if k % 5 != 2 and reqs[k][2] != 7]
        deliver += [deliver[10], deliver[200]]
        sent_pn = {}
        for k in deliver:
            sent_pn.setdefault(reqs[k][2], set()).add(a.want.pn_out[k])
        touched = sorted(sent_pn)
        assert touched == [c for c in range(LOOP_CONNS) if c != 7] and max(sent_pn[0]) - min(sent_pn[0]) > 64
        # B: parse, open by key phase, track
        m = len(deliver)
        dg = np.array([(reqs[k][1], a.want.pkt_len[k], 0) for k in deliver], dtype=ptls_hip.QUIC_DATAGRAM_DTYPE)
        cids = ptls_hip.QuicCidMap(engine, LOOP_CONNS)
        made.append(cids)
        cids.set(LOOP_CIDS, list(range(LOOP_CONNS)))
        rx_b = receiver(m, m)
        d_buf = a.d_pkt.clone()
        d_spaces = i64([0] * (6 * LOOP_CONNS) + [SPACE_SENT] * 16)
        d_expected = i64([0] * (3 * LOOP_CONNS))
        assert rx_b.parse(dg, d_buf, call.buf_len, cidmap=cids, short_cid_len=8, expected_pn=d_expected, expected_count=3 * LOOP_CONNS) == m
        d_out = torch.full((call.buf_len,), FILL, dtype=torch.uint8, device="cuda")
        d_sel, d_gen = u32(np.full(m + 8, SEL_SENT)), u32(np.full(m + 8, GEN_SENT))
        d_res, d_pn = i64([SENTINEL] * (m + 8)), i64([SENTINEL] * (m + 8))
        d_phase = dev(phase_table(gens, first_pn=0).view(np.uint8))
        rep = rx_b.open_keyphase(keys.ks, keys.hp, d_phase, LOOP_CONNS, LOOP_CONNS, d_gen, d_buf, call.buf_len, d_out, call.buf_len, d_sel,
                                 d_res, d_pn)
        assert rep.n_selected == m
        d_verdict, d_touched = u32(np.full(m + 8, VERDICT_SENT)), u32(np.full(LOOP_CONNS + 8, TOUCHED_SENT))
        n = rx_b.track(d_spaces, LOOP_CONNS, d_sel, d_res, d_pn, d_verdict, d_touched, d_expected, 3 * LOOP_CONNS)
        torch.cuda.synchronize()
        assert read_u64(d_res)[:m] == [reqs[k][3] for k in deliver] and read_u64(d_pn)[:m] == [a.want.pn_out[k] for k in deliver]
        new, dup = ptls_hip.QUIC_PN_NEW, ptls_hip.QUIC_PN_DUPLICATE
        assert read_u32(d_verdict)[:m].tolist() == [new] * (m - 2) + [dup] * 2
        assert n == len(touched) and read_u32(d_touched)[:n].tolist() == touched
        # B: the frames and the requests, from d_touched as it is
        after = read_u64(d_spaces)
        spaces = [after[2 * p: 2 * p + 2] for p in range(3 * LOOP_CONNS)]
        in_off, base, stride = 37, 9, 128
        in_len_b = in_off + model.ACK_MAX * n
        d_in = torch.full((in_len_b + 16,), FILL, dtype=torch.uint8, device="cuda")
        d_status, d_off, d_len = u32(np.full(n + 8, STATUS_SENT)), u32(np.full(n + 8, OFF_SENT)), u32(np.full(n + 8, LEN_SENT))
        d_reqs = torch.full(((n + 4) * REQ.itemsize,), REQ_FILL, dtype=torch.uint8, device="cuda")
        ack = rx_b.ack(d_spaces, LOOP_CONNS, 2, d_touched, n, d_in[in_off:], model.ACK_MAX * n, d_status, d_off, d_len, d_reqs, ack_delay=25,
                       in_off=in_off, pkt_base=base, pkt_stride=stride)
        torch.cuda.synchronize()
        want = model.ack(spaces, LOOP_CONNS, 2, touched, 25, 31, in_off, base, stride)
        assert want.status == [OK] * n and read_u32(d_status)[:n].tolist() == want.status
        assert (ack.n_frames, ack.bytes) == (n, len(want.bytes)) and read_u64(d_spaces) == after
        h_in = d_in.cpu().numpy()
        assert h_in[in_off: in_off + ack.bytes].tobytes() == want.bytes
        assert (h_in[:in_off] == FILL).all() and (h_in[in_off + ack.bytes:] == FILL).all()
        assert d_reqs.cpu().numpy()[:n * REQ.itemsize].tobytes() == req_rows(want.reqs).tobytes()
        # B: sealed from the requests as they came out
        b_conns = [Conn(next_pn=40 + c, gen=0, dcid=LOOP_CIDS[c]) for c in range(LOOP_CONNS)]
        d_bconns = dev(conn_table(b_conns).view(np.uint8).copy())
        tx_b = ptls_hip.QuicTx(engine, n)
        made.append(tx_b)
        buf_len_b = base + n * stride
        d_pkt = torch.full((buf_len_b + SPARE,), FILL, dtype=torch.uint8, device="cuda")
        d_tx_status, d_tx_len, d_tx_pn = u32(np.full(n + 8, STATUS_SENT)), u32(np.full(n + 8, LEN_SENT)), i64([SENTINEL] * (n + 8))
        sealed = tx_b.seal(keys.ks, keys.hp, d_bconns, LOOP_CONNS, LOOP_CONNS, d_reqs, ack.n_frames, d_in, in_len_b, d_pkt, buf_len_b,
                           d_tx_status, d_tx_pn, d_tx_len)
        torch.cuda.synchronize()
        assert sealed.n_sent == n and read_u32(d_tx_status)[:n].tolist() == [ptls_hip.QUIC_TX_SENT] * n
        assert read_u64(d_tx_pn)[:n] == [40 + c for c in touched]
        pkt_len = read_u32(d_tx_len)[:n].tolist()
        assert pkt_len == [1 + 8 + 1 + k + 16 for k in want.frame_len]
        # A: parse, open; the plaintexts are the frames
        dg2 = np.array([(base + j * stride, pkt_len[j], 0) for j in range(n)], dtype=ptls_hip.QUIC_DATAGRAM_DTYPE)
        rx_a = receiver(n, n)
        assert rx_a.parse(dg2, d_pkt, buf_len_b, cidmap=cids, short_cid_len=8, expected_pn=i64([0] * (3 * LOOP_CONNS)),
                          expected_count=3 * LOOP_CONNS) == n
        d_out2 = torch.full((buf_len_b,), FILL, dtype=torch.uint8, device="cuda")
        d_sel2, d_res2, d_pn2 = u32(np.full(n + 8, SEL_SENT)), i64([SENTINEL] * (n + 8)), i64([SENTINEL] * (n + 8))
        rep2 = rx_a.open(keys.ks, keys.hp, d_pkt, buf_len_b, d_out2, buf_len_b, d_sel2, d_res2, d_pn2)
        torch.cuda.synchronize()
        assert rep2.n_selected == n and read_u64(d_res2)[:n] == want.frame_len and read_u32(d_sel2)[:n].tolist() == list(range(n))
        pkts, out = rx_a.packets(), d_out2.cpu().numpy()
        for j, c in enumerate(touched):
            assert int(pkts["key"][j]) == c
            plain = out[int(pkts["data_off"][j]): int(pkts["data_off"][j]) + want.frame_len[j]].tobytes()
            assert plain == want.frames[j]
            largest, delay, ranges, end = gen.decode(plain)
            assert end == len(plain) and delay == 25 and largest == max(sent_pn[c])
            assert gen.acknowledged(ranges) == {pn for pn in sent_pn[c] if largest - pn < 64}
        assert len(gen.decode(want.frames[0])[2]) > 10  # (connection 0: a run of four between every dropped packet)
    finally:
        torch.cuda.synchronize()
        for x in reversed(made):
            x.close()
        keys.close()


# ---- refusals ----

def test_refusals_and_nothing_listed(receiver):
    """every refusal of rx_ack with a real receive object and real arrays: nothing launched, nothing written; a call with
    nothing listed returns 0 with both sums 0 and writes nothing"""
    rx = receiver()
    call = gen.sized_call(40)
    arrays = Arrays(call)
    L, P = ptls_hip.lib(), ptls_hip._ptr
    rep = ptls_hip.QuicRxAckReport(77, 77)
    top, most = (1 << 64) - 1, 0xFFFFFFFF // 81
    base = dict(d_spaces=P(arrays.d_spaces), count=call.count, space=2, max_ranges=31, ack_delay=0, d_frames=P(arrays.d_frames),
                frames_len=arrays.frames_len, in_off=0, pkt_base=0, pkt_stride=0, d_status=P(arrays.d_status), d_frame_off=P(arrays.d_off),
                d_frame_len=P(arrays.d_len), d_reqs=P(arrays.d_reqs))
    fields = [f for f, _ in ptls_hip.QuicRxAck._fields_]

    def ack(obj=rx.ptr, null_params=False, d_list=P(arrays.d_list), n=arrays.n, report=rep, **kw):
        p = ptls_hip.QuicRxAck(*[dict(base, **kw)[f] for f in fields])
        return L.ptls_hip_quic_rx_ack(obj, None if null_params else ctypes.addressof(p), d_list, n,
                                      ctypes.addressof(report) if report is not None else None, None)

    refusals = [(dict(obj=None), "null receive object, parameters or report"), (dict(null_params=True), "null receive object"),
                (dict(report=None), "null receive object"), (dict(d_spaces=None), "null state, status"), (dict(d_status=None), "null state, status"),
                (dict(d_frame_off=None), "null state, status"), (dict(d_frame_len=None), "null state, status"),
                (dict(d_reqs=None), "null state, status"), (dict(d_list=None), "null list or frame buffer"),
                (dict(d_frames=None), "null list or frame buffer"), (dict(count=0), "a connection count of 0 is outside"),
                (dict(count=1 << 32), "a connection count of 4294967296 is outside"), (dict(space=3), "packet-number space 3 is above 2"),
                (dict(ack_delay=1 << 62), "is not below 2^62"), (dict(n=most + 1, frames_len=top), "do not fit the 32-bit scan levels"),
                (dict(frames_len=arrays.frames_len - 1), "a frame buffer of %d bytes is below 81 for each of the 40" % (arrays.frames_len - 1)),
                (dict(in_off=top - 81 * 40 + 1), "in_off plus 81 bytes for each of the 40 list entries wraps 2^64"),
                (dict(pkt_base=top - 39, pkt_stride=1), "pkt_base plus 40 packets of stride 1 wraps 2^64"),
                (dict(pkt_stride=1 << 60), "pkt_base plus 40 packets of stride 1152921504606846976 wraps 2^64")]
    for kw, msg in refusals:
        assert ack(**kw) == ptls_hip.EINVAL, kw
        assert "quic_rx_ack:" in ptls_hip.last_error() and msg in ptls_hip.last_error(), (kw, ptls_hip.last_error())
        assert (rep.n_frames, rep.bytes) == (77, 77)
    torch.cuda.synchronize()
    arrays.untouched()
    assert ack(n=0) == 0 and (rep.n_frames, rep.bytes) == (0, 0)
    torch.cuda.synchronize()
    arrays.untouched()
    # the same arrays, now for real: the refusals left nothing behind in the object either
    arrays.run(rx).check()
