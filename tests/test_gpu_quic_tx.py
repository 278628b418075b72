"""The send object on the GPU (include/ptls_hip.h 2l; hsig-picotls_amd/csrc/quic_tx_kernel.hip, quic_tx.cpp).  Exact, no
tolerance anywhere: every status, packet number and packet length, the whole state table, the whole packet buffer and the
whole payload buffer against the plain-Python model (tests/quic_tx_ref.py, packet bytes through tests/quic_ref.py), and the
packet buffer again against ptls_hip_quic_seal_batch fed host-written headers and the model's numbers.  The three output
arrays and the state table start sentinel-filled with spare elements (the table's reserved and unused connection-ID bytes
too), the packet buffer 0xA5-filled with 64 spare bytes, and everything is compared whole.  The cases are
tests/quic_tx_cases.py's, which tests/test_quic_tx_ref.py and tests/test_quic_tx_native.py hold against hand-written
statements and the host build of the same code.

Payloads are 20 bytes unless a case says otherwise.  Sizes: 130 connections; 1, 255, 256, 257 and 2 049 requests (the passes'
workgroup is 256 threads); one run of 4 096; runs that begin and end on workgroup edges; 2 047 / 2 048 / 2 049 runs
(QP_SCAN_SPAN = 2048).  The ChaCha20-Poly1305 model is plain Python: where a call has thousands of packets or packets of 64 KiB
it computes a sample of them, and the comparison with ptls_hip_quic_seal_batch covers every byte."""
import ctypes

import numpy as np
import pytest
import torch

import ptls_hip
import quic_ref
import quic_tx_cases as gen
import quic_tx_ref as model
from quic_tx_ref import Conn, NONE_ACKED
from test_gpu_quic import ALGO_OF, FILL, SENTINEL, U64, dev, stream

pytestmark = pytest.mark.gpu
ALGOS = ["aes128", "aes256", "chacha"]
STATUS_SENT, LEN_SENT, SEL_SENT, GEN_SENT, VERDICT_SENT, TOUCHED_SENT = 0xD1D1D1D1, 0xC7C7C7C7, 0xC3C3C3C3, 0xB4B4B4B4, 0xD7D7D7D7, 0xC9C9C9C9
TABLE_FILL, SPARE = 0xEE, 64
SENT = model.SENT


def u32(values):
    return torch.from_numpy(np.array(values, dtype=np.uint32).view(np.int32)).cuda()


def read_u32(t):
    return t.cpu().numpy().view(np.uint32)


def read_u64(t):
    return [int(x) & U64 for x in t.cpu().tolist()]


class TxKeys:
    """3 * stride AEAD slots (the three banks) and hp_slots header-protection slots, every slot with a key of its own"""

    def __init__(self, engine, algo, stride, hp_slots):
        kind, ksz = ALGO_OF[algo]
        self.algo, self.stride, self.hp_slots, n = algo, stride, hp_slots, 3 * stride
        self.keys = [stream("gpu-quic-tx-%s-key-%d" % (algo, s), ksz) for s in range(n)]
        self.ivs = [stream("gpu-quic-tx-%s-iv-%d" % (algo, s), 12) for s in range(n)]
        self.hps = [stream("gpu-quic-tx-%s-hp-%d" % (algo, c), ksz) for c in range(hp_slots)]
        self.ks, self.hp = ptls_hip.KeySet(engine, ksz, n, algo=kind), ptls_hip.KeySet(engine, ksz, hp_slots, algo=kind)
        self.ks.set(0, b"".join(self.keys), b"".join(self.ivs))
        self.hp.set(0, b"".join(self.hps), None)

    def close(self):
        self.ks.close()
        self.hp.close()


@pytest.fixture(scope="module")
def keyed(engine):
    made = {}

    def get(algo, stride=gen.STRIDE, hp_slots=gen.HP_SLOTS):
        if (algo, stride, hp_slots) not in made:
            made[algo, stride, hp_slots] = TxKeys(engine, algo, stride, hp_slots)
        return made[algo, stride, hp_slots]

    yield get
    torch.cuda.synchronize()
    for k in made.values():
        k.close()


@pytest.fixture
def sender(engine):
    made = []

    def make(cap):
        made.append(ptls_hip.QuicTx(engine, cap))
        return made[-1]

    yield make
    torch.cuda.synchronize()
    for tx in made:
        tx.close()


def conn_table(conns, spare=2):
    """the state table with `spare` entries behind it; every byte the model does not name is TABLE_FILL"""
    t = np.full((len(conns) + spare) * ptls_hip.QUIC_TXCONN_DTYPE.itemsize, TABLE_FILL, np.uint8).view(ptls_hip.QUIC_TXCONN_DTYPE)
    for c, k in enumerate(conns):
        t["next_pn"][c], t["largest_acked"][c], t["gen"][c] = np.uint64(k.next_pn), np.uint64(k.largest_acked), k.gen
        t["dcid_len"][c], t["flags"][c] = k.dcid_len, k.flags
        t["dcid"][c][:len(k.dcid)] = np.frombuffer(k.dcid, np.uint8)
    return t


def phase_table(gens, first_pn=U64):
    t = np.zeros(len(gens), dtype=ptls_hip.QUIC_KEYPHASE_DTYPE)
    t["gen"], t["first_pn"] = gens, np.uint64(first_pn)
    return t


def req_array(reqs):
    a = np.zeros(len(reqs), dtype=ptls_hip.QUIC_TXREQ_DTYPE)
    a["data_off"] = np.array([r[0] for r in reqs], dtype=np.uint64)
    a["pkt_off"] = np.array([r[1] for r in reqs], dtype=np.uint64)
    a["conn"], a["len"] = [r[2] for r in reqs], [r[3] for r in reqs]
    return a


def payload_buffer(call):
    return np.frombuffer(stream("gpu-quic-tx-payload", call.in_len), np.uint8).copy()


def descriptors(call, o):
    """what a host caller of ptls_hip_quic_seal_batch would upload for the model's sent packets"""
    sent = o.sent
    d = np.zeros(len(sent), dtype=ptls_hip.QUIC_PACKET_DTYPE)
    d["data_off"] = np.array([call.reqs[j][0] for j in sent], dtype=np.uint64)
    d["pkt_off"] = np.array([call.reqs[j][1] for j in sent], dtype=np.uint64)
    d["pn"] = np.array([o.pn_out[j] for j in sent], dtype=np.uint64)
    d["pkt_len"], d["key"], d["hp_key"] = [o.pkt_len[j] for j in sent], [o.slots[j] for j in sent], [call.reqs[j][2] for j in sent]
    d["pn_len"] = [(o.headers[j][0] & 3) + 1 for j in sent]
    d["pn_offset"] = [len(o.headers[j]) - (o.headers[j][0] & 3) - 1 for j in sent]
    return d


class Sealed:
    """one tx.seal() of a Call with fresh sentinel-filled arrays (or the device state table of a call before), everything read
    back and compared whole with the model; want: the model's outcome"""

    def __init__(self, engine, tx, keys, call, d_conns=None, conns=None, d_rx_phase=None, model_every=1, model_max=1 << 20):
        self.call, n = call, len(call.reqs)
        conns = call.conns if conns is None else conns
        self.want = o = call.want(conns)
        self.table_before = conn_table(conns[:call.count])
        self.d_conns = dev(self.table_before.view(np.uint8).copy()) if d_conns is None else d_conns
        if d_rx_phase is None and call.rx_gens is not None:
            d_rx_phase = dev(phase_table(call.rx_gens[:call.count]).view(np.uint8))
        self.h_in = payload_buffer(call)
        self.d_in = dev(self.h_in.copy())
        self.d_pkt = torch.full((call.buf_len + SPARE,), FILL, dtype=torch.uint8, device="cuda")
        self.d_status, self.d_len = u32(np.full(n + 8, STATUS_SENT)), u32(np.full(n + 8, LEN_SENT))
        self.d_pn = torch.full((n + 8,), SENTINEL, dtype=torch.int64, device="cuda")
        self.d_reqs = dev(req_array(call.reqs).view(np.uint8))
        self.rep = tx.seal(keys.ks, keys.hp, self.d_conns, call.count, call.stride, self.d_reqs, n, self.d_in, call.in_len, self.d_pkt,
                           call.buf_len, self.d_status, self.d_pn, self.d_len, d_rx_phase=d_rx_phase, pn_len=call.pn_len)
        torch.cuda.synchronize()
        # the three arrays, exactly n elements each
        status, lens, pns = read_u32(self.d_status), read_u32(self.d_len), read_u64(self.d_pn)
        assert (status[n:] == STATUS_SENT).all() and (lens[n:] == LEN_SENT).all() and pns[n:] == [SENTINEL] * 8
        self.status, self.pkt_len, self.pn_out = status[:n].tolist(), lens[:n].tolist(), pns[:n]
        assert self.status == o.status, next((j, g, w) for j, (g, w) in enumerate(zip(self.status, o.status)) if g != w)
        assert self.pn_out == o.pn_out, next((j, g, w) for j, (g, w) in enumerate(zip(self.pn_out, o.pn_out)) if g != w)
        assert self.pkt_len == o.pkt_len
        sent = o.sent
        assert self.rep.n_sent == len(sent) == len(tx) and self.rep.bytes == sum(o.pkt_len)
        assert self.rep.lanes in ((0,) if not sent else (64,) if keys.algo != "chacha" else (1, 4, 16, 64))
        # the state table, whole: next_pn and gen of the numbered connections, every other byte as it was
        want_table = self.table_before.copy()
        for c in range(call.count):
            want_table["next_pn"][c], want_table["gen"][c] = np.uint64(o.conns[c].next_pn), o.conns[c].gen
        self.table = self.d_conns.cpu().numpy().view(ptls_hip.QUIC_TXCONN_DTYPE)
        if d_conns is None:
            assert self.table.tobytes() == want_table.tobytes()
        # the payloads are not written; the packed descriptors are the host caller's
        assert np.array_equal(self.d_in.cpu().numpy(), self.h_in)
        desc = descriptors(call, o)
        assert tx.packets().tobytes() == desc.tobytes()
        # the packet buffer, whole: against ptls_hip_quic_seal_batch over host-written headers ...
        self.pkt = self.d_pkt.cpu().numpy()
        assert (self.pkt[call.buf_len:] == FILL).all()
        h_hdr = np.full(call.buf_len + SPARE, FILL, np.uint8)
        for j in sent:
            h_hdr[call.reqs[j][1]: call.reqs[j][1] + len(o.headers[j])] = np.frombuffer(o.headers[j], np.uint8)
        if sent:
            d_pkt2 = dev(h_hdr.copy())
            q = ptls_hip.QuicBatch(engine, desc, open=False)
            try:
                q.seal(keys.ks, keys.hp, self.d_in, d_pkt2)
                torch.cuda.synchronize()
            finally:
                q.close()
            assert np.array_equal(self.pkt, d_pkt2.cpu().numpy())
        # ... and against the model: the picked packets byte for byte, and nothing outside the sent packets
        outside, one_long = np.ones(call.buf_len + SPARE, bool), False
        for k, j in enumerate(sent):
            off, length = call.reqs[j][1], o.pkt_len[j]
            outside[off: off + length] = False
            if k % model_every == 0 and (length <= model_max or not one_long):
                one_long = one_long or length > model_max
                pay = self.h_in[call.reqs[j][0]: call.reqs[j][0] + call.reqs[j][3]].tobytes()
                conn = call.reqs[j][2]
                want = model.packet(keys.algo, keys.keys[o.slots[j]], keys.ivs[o.slots[j]], keys.hps[conn], o.headers[j], o.pn_out[j], pay)
                assert self.pkt[off: off + length].tobytes() == want, (j, conn)
        assert (self.pkt[outside] == FILL).all()


# ---- the shared cases ----

@pytest.mark.parametrize("algo,pn_len,rx", [("aes128", 0, None), ("aes256", 2, "mixed"), ("chacha", 0, "mixed"), ("aes128", 4, None),
                                            ("chacha", 1, None), ("aes256", 3, None)])
def test_the_case_list(engine, keyed, sender, algo, pn_len, rx):
    """every state and every refusal over 130 connections, the connections in no ascending order; packets of 65 535 bytes among
    them, the last packet ending with the buffer's last byte"""
    call = gen.case_list(pn_len, rx)
    s = Sealed(engine, sender(len(call.reqs)), keyed(algo), call, model_max=4096 if algo == "chacha" else 1 << 20)
    assert set(s.status) == {model.SENT, model.NO_CONN, model.SPLIT, model.PN, model.RANGE}
    assert max(s.pkt_len) <= 65535 and (pn_len > 2 or 65535 in s.pkt_len)


@pytest.mark.parametrize("what,value", [("count", 60), ("stride", 100), ("hp_slots", 7)])
def test_the_three_bounds_of_a_connection(engine, keyed, sender, what, value):
    """a smaller state count, a smaller bank stride, a smaller header-protection keyset: connections at and above each are
    NO_CONN and their state entries untouched (the object's per-connection scratch shrinks and grows between the calls)"""
    tx = sender(400)
    full = gen.case_list(0)
    keys = keyed("aes128") if what == "count" else keyed("aes128", value, gen.HP_SLOTS) if what == "stride" else keyed("aes128", gen.STRIDE, value)
    s = Sealed(engine, tx, keys, full.with_(**{what: value}))
    assert s.status.count(model.NO_CONN) > 40
    Sealed(engine, tx, keyed("aes128"), full)


# ---- sizes ----

@pytest.mark.parametrize("n,algo", [(1, "aes128"), (255, "chacha"), (256, "aes256"), (257, "aes128"), (2049, "chacha")])
def test_request_counts(engine, keyed, sender, n, algo):
    s = Sealed(engine, sender(2049), keyed(algo), gen.sized_call(n), model_every=1 if algo != "chacha" else 16)
    assert s.status == [SENT] * n


@pytest.mark.parametrize("algo", ["aes128", "chacha"])
def test_one_run_across_workgroups(engine, keyed, sender, algo):
    """4 096 requests of one connection: the numbers are a plain position difference from one head"""
    call = gen.one_run_call(4096)
    s = Sealed(engine, sender(4096), keyed(algo), call, model_every=1 if algo != "chacha" else 64)
    base = call.conns[0].next_pn
    assert s.pn_out == list(range(base, base + 4096)) and int(s.table["next_pn"][0]) == base + 4096


def test_runs_on_workgroup_edges(engine, keyed, sender):
    call = gen.edges_call()
    s = Sealed(engine, sender(len(call.reqs)), keyed("aes256"), call)
    assert s.status == [SENT] * len(call.reqs)


@pytest.mark.parametrize("k", [2047, 2048, 2049])
def test_run_counts_across_the_scan_span(engine, keyed, sender, k):
    call = gen.many_runs_call(k)
    s = Sealed(engine, sender(2049), keyed("chacha", 2056, 2056), call, model_every=64)
    assert s.status == [SENT] * k and s.rep.n_sent == k


@pytest.mark.parametrize("algo", ALGOS)
def test_payload_lengths(engine, keyed, sender, algo):
    """3, 15, 16, 17 and 1 350 bytes and the longest payload, packets at odd byte offsets"""
    call = gen.lengths_call()
    s = Sealed(engine, sender(len(call.reqs)), keyed(algo), call)
    assert s.status == [SENT] * len(call.reqs) and 65535 in s.pkt_len
    assert all(r[1] % 2 == 1 for r in call.reqs)


# ---- the state stays on the device ----

@pytest.mark.parametrize("algo", ["aes128", "chacha"])
def test_two_calls_in_a_row(engine, keyed, sender, algo):
    """the second call works from the table the first one left, with no host write in between: the numbers continue"""
    call = gen.sized_call(257)
    tx, keys = sender(257), keyed(algo)
    a = Sealed(engine, tx, keys, call)
    b = Sealed(engine, tx, keys, call, d_conns=a.d_conns, conns=a.want.conns)
    assert b.status == [SENT] * 257 and all(y > x for x, y in zip(a.pn_out, b.pn_out))
    want_table = a.table_before.copy()
    for c in range(call.count):
        want_table["next_pn"][c], want_table["gen"][c] = np.uint64(b.want.conns[c].next_pn), b.want.conns[c].gen
    assert b.table.tobytes() == want_table.tobytes()
    by_conn = {}
    for r, x, y in zip(call.reqs, a.pn_out, b.pn_out):
        by_conn.setdefault(r[2], []).append((x, y))
    for pairs in by_conn.values():
        nums = [x for x, _ in pairs] + [y for _, y in pairs]
        assert nums == list(range(nums[0], nums[0] + len(nums)))


# ---- the loop closed: tx packets through the peer's parse, open by key phase, and track ----

LOOP_CONNS = 12
LOOP_CIDS = [bytes([0xB0 + c]) + bytes(range(c, c + 7)) for c in range(LOOP_CONNS)]


def loop_conns(gens):
    return [Conn(next_pn=1000 + 50 * c, largest_acked=1000 + 50 * c - 1 - c, gen=gens[c], dcid=LOOP_CIDS[c], flags=c & 1)
            for c in range(LOOP_CONNS)]


def loop_call(conns, per_conn=3, payload=gen.PAYLOAD):
    items = []
    for c in range(LOOP_CONNS):
        items += [((c * 5) % LOOP_CONNS, payload + c)] * per_conn
    reqs, in_len, buf_len = gen.lay_out(items)
    return gen.Call(conns, reqs, in_len, buf_len, stride=LOOP_CONNS, hp_slots=LOOP_CONNS)


class Peer:
    """the receiving end: the connection-ID map, the key-phase table, the packet-number spaces and the expected-pn table, in
    device memory; it has received every packet up to the sender's largest_acked"""

    def __init__(self, engine, keys, conns, gens):
        self.engine, self.keys = engine, keys
        self.map = ptls_hip.QuicCidMap(engine, LOOP_CONNS)
        self.map.set(LOOP_CIDS, list(range(LOOP_CONNS)))
        self.d_phase = dev(phase_table(gens, first_pn=0).view(np.uint8))
        spaces, expected = [], []
        for k in conns:
            nxt = 0 if k.largest_acked == NONE_ACKED else k.largest_acked + 1
            spaces += [0, 0, 0, 0, nxt, U64 if nxt else 0]
            expected += [0, 0, nxt]
        self.d_spaces = torch.tensor(np.array(spaces, dtype=np.uint64).view(np.int64), device="cuda")
        self.d_expected = torch.tensor(np.array(expected, dtype=np.uint64).view(np.int64), device="cuda")

    def close(self):
        torch.cuda.synchronize()
        self.map.close()

    def receive(self, s):
        """the sent packets of a Sealed as datagrams: parse, open by key phase, track; (results, packet numbers, generations,
        verdicts, plaintexts)"""
        call, o = s.call, s.want
        sent = o.sent
        dg = np.array([(call.reqs[j][1], o.pkt_len[j], 0) for j in sent], dtype=ptls_hip.QUIC_DATAGRAM_DTYPE)
        m, total = len(sent), call.buf_len
        rx = ptls_hip.QuicRx(self.engine, m, m)
        try:
            d_buf = s.d_pkt.clone()
            assert rx.parse(dg, d_buf, total, cidmap=self.map, short_cid_len=8, expected_pn=self.d_expected,
                            expected_count=3 * LOOP_CONNS) == m
            d_out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
            d_sel, d_gen = u32(np.full(m + 8, SEL_SENT)), u32(np.full(m + 8, GEN_SENT))
            d_res = torch.full((m + 8,), SENTINEL, dtype=torch.int64, device="cuda")
            d_pn = torch.full((m + 8,), SENTINEL, dtype=torch.int64, device="cuda")
            rep = rx.open_keyphase(self.keys.ks, self.keys.hp, self.d_phase, LOOP_CONNS, LOOP_CONNS, d_gen, d_buf, total, d_out, total,
                                   d_sel, d_res, d_pn)
            assert rep.n_selected == m
            d_updated = u32(np.full(LOOP_CONNS + 8, TOUCHED_SENT))
            self.updated = rx.keyphase_commit(self.d_phase, LOOP_CONNS, d_res, d_pn, d_gen, d_updated)
            d_verdict, d_touched = u32(np.full(m + 8, VERDICT_SENT)), u32(np.full(LOOP_CONNS + 8, TOUCHED_SENT))
            rx.track(self.d_spaces, LOOP_CONNS, d_sel, d_res, d_pn, d_verdict, d_touched, self.d_expected, 3 * LOOP_CONNS)
            torch.cuda.synchronize()
            pkts = rx.packets()
            out = d_out.cpu().numpy()
            plain = [out[int(p["data_off"]): int(p["data_off"]) + call.reqs[j][3]].tobytes() for p, j in zip(pkts, sent)]
            return (read_u64(d_res)[:m], read_u64(d_pn)[:m], read_u32(d_gen)[:m].tolist(), read_u32(d_verdict)[:m].tolist(), plain)
        finally:
            torch.cuda.synchronize()
            rx.close()


def check_received(s, got, gens):
    call, o = s.call, s.want
    res, pns, got_gens, verdicts, plain = got
    sent = o.sent
    assert res == [call.reqs[j][3] for j in sent] and pns == [o.pn_out[j] for j in sent]
    assert got_gens == [gens[call.reqs[j][2]] for j in sent]
    assert verdicts == [ptls_hip.QUIC_PN_NEW] * len(sent)
    assert plain == [s.h_in[call.reqs[j][0]: call.reqs[j][0] + call.reqs[j][3]].tobytes() for j in sent]


@pytest.mark.parametrize("algo", ALGOS)
def test_the_loop_closed(engine, sender, algo):
    """what tx_seal wrote goes through rx_parse, rx_open_keyphase and rx_track on a peer's tables: every packet opens under its
    generation's bank, is new, and every plaintext is the payload; a second call on the same tables continues"""
    keys = TxKeys(engine, algo, LOOP_CONNS, LOOP_CONNS)
    gens = [c % 4 for c in range(LOOP_CONNS)]
    conns = loop_conns(gens)
    peer = Peer(engine, keys, conns, gens)
    try:
        call = loop_call(conns)
        tx = sender(len(call.reqs))
        a = Sealed(engine, tx, keys, call)
        assert a.status == [SENT] * len(call.reqs)
        check_received(a, peer.receive(a), gens)
        b = Sealed(engine, tx, keys, call, d_conns=a.d_conns, conns=a.want.conns)
        check_received(b, peer.receive(b), gens)
        assert peer.updated == 0
    finally:
        peer.close()
        torch.cuda.synchronize()
        keys.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_key_update_followed(engine, sender, algo):
    """the peer updates its keys on half of the connections: its packets of generation g + 1 are opened here by key phase and the
    update is committed on the device (2j); the next tx_seal with that state array sends those connections in the new phase and
    stores the generation, the others as before, and the peer opens everything"""
    keys = TxKeys(engine, algo, LOOP_CONNS, LOOP_CONNS)
    gens = [c % 3 for c in range(LOOP_CONNS)]
    updating = [c for c in range(LOOP_CONNS) if c % 2 == 0]
    new_gens = [g + 1 if c in updating else g for c, g in enumerate(gens)]
    conns = loop_conns(gens)
    # what the peer sends: one packet per connection, under its new generation's keys (the test's keys are the same both ways)
    their = [Conn(next_pn=70 + c, largest_acked=69 + c, gen=new_gens[c], dcid=LOOP_CIDS[c]) for c in range(LOOP_CONNS)]
    incoming = loop_call(their, per_conn=1)
    ours = Peer(engine, keys, their, gens)  # our receive side: still at the old generations
    theirs = Peer(engine, keys, conns, new_gens)
    try:
        tx = sender(len(loop_call(conns).reqs))
        got = ours.receive(Sealed(engine, tx, keys, incoming))
        assert got[2] == [new_gens[r[2]] for r in incoming.reqs] and U64 not in got[0]
        assert ours.updated == len(updating)
        table = ours.d_phase.cpu().numpy().view(ptls_hip.QUIC_KEYPHASE_DTYPE)
        assert table["gen"].tolist() == new_gens
        # our send side follows with no host step
        call = loop_call(conns)
        s = Sealed(engine, tx, keys, call.with_(rx_gens=new_gens), d_rx_phase=ours.d_phase)
        assert s.table["gen"][:LOOP_CONNS].tolist() == new_gens
        for j in s.want.sent:
            c = call.reqs[j][2]
            assert (s.want.headers[j][0] >> 2) & 1 == new_gens[c] & 1 and s.want.slots[j] == c + LOOP_CONNS * (new_gens[c] % 3)
        check_received(s, theirs.receive(s), new_gens)
        # without the state array the same call would have stayed in the old phase
        old = call.want()
        assert [old.gens[j] for j in old.sent] == [gens[call.reqs[j][2]] for j in old.sent]
    finally:
        ours.close()
        theirs.close()
        torch.cuda.synchronize()
        keys.close()


# ---- refusals ----

def test_refusals_write_nothing(engine, keyed, sender):
    """every refusal of tx_seal with real objects: nothing launched, no byte of any array, of the state table or of the buffers
    touched; then the well-formed call goes through"""
    L, P = ptls_hip.lib(), ptls_hip._ptr
    keys, other = keyed("aes128"), keyed("aes256")
    chacha = keyed("chacha")
    call = gen.sized_call(40)
    n = len(call.reqs)
    tx = sender(n)
    table = conn_table(call.conns)
    d_conns, d_reqs = dev(table.view(np.uint8).copy()), dev(req_array(call.reqs).view(np.uint8))
    d_status, d_len = u32(np.full(n + 8, STATUS_SENT)), u32(np.full(n + 8, LEN_SENT))
    d_pn = torch.full((n + 8,), SENTINEL, dtype=torch.int64, device="cuda")
    d_buf = torch.full((call.in_len + call.buf_len,), FILL, dtype=torch.uint8, device="cuda")  # payloads, then packets
    d_in, d_pkt = d_buf[:call.in_len], d_buf[call.in_len:]
    rep = ptls_hip.QuicTxReport(77, 77, 77, 77)

    def seal(obj=tx.ptr, ks=keys.ks.ptr, hp=keys.hp.ptr, conns=d_conns, count=call.count, stride=call.stride, pn_len=0, reserved=0,
             status=d_status, pn=d_pn, lens=d_len, null_pr=False, reqs=d_reqs, m=n, inp=d_in, in_len=call.in_len, pkt=d_pkt,
             buf_len=call.buf_len, report=rep):
        pr = ptls_hip.QuicTxParams(P(conns), count, stride, None, pn_len, reserved, P(status), P(pn), P(lens))
        return L.ptls_hip_quic_tx_seal(obj, ks, hp, None if null_pr else ctypes.addressof(pr), P(reqs), m, P(inp), in_len, P(pkt), buf_len,
                                       ctypes.addressof(report) if report is not None else None, None)

    def untouched():
        torch.cuda.synchronize()
        assert (rep.n_sent, rep.bytes, rep.lanes, rep.reserved) == (77, 77, 77, 77)
        assert (read_u32(d_status) == STATUS_SENT).all() and (read_u32(d_len) == LEN_SENT).all() and read_u64(d_pn) == [SENTINEL] * (n + 8)
        assert d_conns.cpu().numpy().tobytes() == table.tobytes() and (d_buf.cpu().numpy() == FILL).all()
        assert len(tx) == 0

    small = ptls_hip.KeySet(engine, 16, 3 * call.stride - 1)
    engine2 = ptls_hip.Engine(0)
    foreign = ptls_hip.KeySet(engine2, 16, 3 * call.stride)
    try:
        refusals = [(dict(obj=None), "null send object"), (dict(ks=None), "null send object, keyset"), (dict(hp=None), "keyset"),
                    (dict(null_pr=True), "parameters"), (dict(report=None), "or report"),
                    (dict(conns=None), "null state"), (dict(status=None), "null state, status"), (dict(pn=None), "packet-number"),
                    (dict(lens=None), "packet-length array"), (dict(m=n + 1), "%d requests, the send object was made for %d" % (n + 1, n)),
                    (dict(count=0), "a state count of 0"), (dict(count=1 << 32), "a state count of 4294967296"),
                    (dict(stride=0), "a bank stride of 0"), (dict(pn_len=5), "pn_len 5 is above 4"), (dict(reserved=3), "params.reserved"),
                    (dict(ks=foreign.ptr), "same engine"), (dict(hp=foreign.ptr), "same engine"),
                    (dict(hp=other.hp.ptr), "algorithm and key size"), (dict(hp=chacha.hp.ptr), "algorithm and key size"),
                    (dict(ks=small.ptr), "three banks of stride %d do not fit the keyset's %d slots" % (call.stride, 3 * call.stride - 1)),
                    (dict(reqs=None), "null request array or buffer"), (dict(inp=None), "null request array or buffer"),
                    (dict(pkt=None), "null request array or buffer"),
                    (dict(buf_len=call.buf_len, pkt=d_buf[call.in_len - 1:]), "overlaps the payload buffer"),
                    (dict(pkt=d_in, inp=d_pkt, in_len=call.in_len + 1), "overlaps the payload buffer"),
                    (dict(pkt=d_in, buf_len=call.in_len), "overlaps the payload buffer")]
        for kw, msg in refusals:
            assert seal(**kw) == ptls_hip.EINVAL, kw
            assert "quic_tx_seal:" in ptls_hip.last_error() and msg in ptls_hip.last_error(), (kw, ptls_hip.last_error())
        untouched()
        assert seal(m=0) == 0 and (rep.n_sent, rep.bytes, rep.lanes) == (0, 0, 0)
        rep.n_sent = rep.bytes = rep.lanes = rep.reserved = 77
        untouched()
        # adjacent buffers are no overlap: the call goes through, and the payload half keeps its fill
        d_buf[:call.in_len] = dev(payload_buffer(call))
        assert seal() == 0 and rep.n_sent == n
        torch.cuda.synchronize()
        assert read_u32(d_status)[:n].tolist() == [SENT] * n and np.array_equal(d_in.cpu().numpy(), payload_buffer(call))
    finally:
        torch.cuda.synchronize()
        small.close()
        foreign.close()
        engine2.close()
