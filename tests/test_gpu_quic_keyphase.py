"""Receive keys chosen by Key Phase bit on the GPU, and key updates committed there (include/ptls_hip.h 2j;
hsig-picotls_amd/csrc/quic_phase_kernel.hip, quic_rx.cpp).  Bit-exact, no tolerance anywhere: the generation of every packet
against the plain-Python model (tests/quic_phase_ref.py), every result, packet number, the whole packet buffer and the whole
0xA5-filled output buffer against the plain-Python packet protection (tests/quic_ref.py) under the one key the model names,
the state table and the list of updated connections after a commit against the model's.  d_sel, d_result, d_pn_out, d_gen_out
and d_updated start sentinel-filled with 8 elements to spare, and what lies behind the elements a call owns must come back
untouched.  The cases are tests/quic_phase_cases.py's, which tests/test_quic_phase_ref.py holds against the reference alone.

Sizes: 130 connections (wave boundaries at 63 / 64 / 65 connections and packets fall inside), a few hundred packets per case;
the header kernel at 1, 255, 256, 257 packets (its workgroup is 256 threads); the commit's compaction at 2 047 / 2 048 / 2 049
connections (QP_SCAN_SPAN = 2048)."""
import ctypes

import numpy as np
import pytest
import torch

import ptls_hip
import quic_phase_cases as gen
import quic_phase_ref as model
import quic_ref
import quic_rx_ref
from test_gpu_quic import ALGO_OF, FILL, NKEYS, SENTINEL, U64, dev, image, key_material, keysets, place, protected, specs  # noqa: F401
from test_gpu_quic_rx import ALL, SEL_SENT, load, spec_input

pytestmark = pytest.mark.gpu
GEN_SENT = 0xB4B4B4B4
NO_GEN = ptls_hip.QUIC_NO_GEN
ALGOS = ["aes128", "aes256", "chacha"]


def u32(values):
    return torch.from_numpy(np.array(values, dtype=np.uint32).view(np.int32)).cuda()


def filler(tag, slot, n):
    return gen.stream("keyphase-filler-%s-%d" % (tag, slot), n)


class Keys:
    """a case's keysets: 3 * stride AEAD slots (the three banks; unkeyed slots hold filler that opens nothing) and its
    header-protection slots"""

    def __init__(self, engine, case, hp_slots=None):
        kind, ksz = ALGO_OF[case.algo]
        self.case, self.ksz = case, ksz
        self.nslots, self.hp_nslots = 3 * case.stride, hp_slots or case.count
        self.ks = ptls_hip.KeySet(engine, ksz, self.nslots, algo=kind)
        self.hp = ptls_hip.KeySet(engine, ksz, self.hp_nslots, algo=kind)
        self.hps = [case.hps[c] if c < len(case.hps) else filler("hp", c, ksz) for c in range(self.hp_nslots)]
        self.hp.set(0, b"".join(self.hps), None)
        self.set_banks(case)

    def set_banks(self, case):
        """the three banks as `case`'s states have them (after a key update: the bank of generation gen - 2 re-keyed)"""
        self.table = {s: (filler("key", s, self.ksz), filler("iv", s, 12)) for s in range(self.nslots)}
        self.table.update(case.slot_keys())
        self.ks.set(0, b"".join(self.table[s][0] for s in range(self.nslots)), b"".join(self.table[s][1] for s in range(self.nslots)))

    def close(self):
        torch.cuda.synchronize()
        self.ks.close()
        self.hp.close()


@pytest.fixture
def keyed(engine):
    made = []

    def make(case, **kw):
        made.append(Keys(engine, case, **kw))
        return made[-1]

    yield make
    for k in made:
        k.close()


def lay_out(case, packets=None, unprotected=False):
    """the packets in a 0xA5-filled buffer at odd offsets with gaps, and their descriptors (key = hp_key = the connection):
    (buffer, descriptors, buffer bytes, output bytes).  unprotected: the headers as the sender wrote them, and the flag"""
    packets = case.packets if packets is None else packets
    raw = [case.protected(p) for p in packets]
    if unprotected:
        raw = [p.header + b[len(p.header):] for p, b in zip(packets, raw)]
    pkt_offs, pkt_total = place([p.pkt_len for p in packets])
    out_offs, out_total = place([len(p.payload) + 4 for p in packets])
    d = np.zeros(len(packets), dtype=ptls_hip.QUIC_PACKET_DTYPE)
    d["pkt_off"], d["data_off"] = pkt_offs, out_offs
    d["pn"] = [p.expected for p in packets]
    d["pkt_len"] = [p.pkt_len for p in packets]
    d["key"] = d["hp_key"] = [p.conn for p in packets]
    d["pn_offset"] = [p.pn_offset for p in packets]
    d["pn_len"] = 9  # open ignores it
    d["flags"] = ptls_hip.QUIC_UNPROTECTED if unprotected else 0
    return image(pkt_total, pkt_offs, raw), d, pkt_total, out_total


def phase_table(states):
    t = np.zeros(len(states), dtype=ptls_hip.QUIC_KEYPHASE_DTYPE)
    t["gen"], t["first_pn"] = [s[0] for s in states], np.array([s[1] for s in states], dtype=np.uint64)
    return t


def read_table(d_phase):
    t = d_phase.cpu().numpy().view(ptls_hip.QUIC_KEYPHASE_DTYPE)
    assert (t["reserved"] == 0).all()
    return [[int(g), int(f)] for g, f in zip(t["gen"], t["first_pn"])]


class Opened:
    """one rx.open_keyphase() (plain=True: rx.open()) with fresh sentinel-filled arrays: everything read back"""

    def __init__(self, rx, keys, d_phase, count, stride, d_buf, buf_len, out_total, plain=False, mask=ALL):
        cap = len(rx) + 8
        d_out = torch.full((out_total,), FILL, dtype=torch.uint8, device="cuda")
        d_sel = u32(np.full(cap, SEL_SENT))
        self.d_res = torch.full((cap,), SENTINEL, dtype=torch.int64, device="cuda")
        self.d_pn = torch.full((cap,), SENTINEL, dtype=torch.int64, device="cuda")
        self.d_gen = u32(np.full(cap, GEN_SENT))
        if plain:
            self.rep = rx.open(keys.ks, keys.hp, d_buf, buf_len, d_out, out_total, d_sel, self.d_res, self.d_pn, type_mask=mask)
        else:
            self.rep = rx.open_keyphase(keys.ks, keys.hp, d_phase, count, stride, self.d_gen, d_buf, buf_len, d_out, out_total, d_sel,
                                        self.d_res, self.d_pn, type_mask=mask)
        torch.cuda.synchronize()
        self.m = m = int(self.rep.n_selected)
        sel = d_sel.cpu().numpy().view(np.uint32)
        gens = self.d_gen.cpu().numpy().view(np.uint32)
        res = [int(x) & U64 for x in self.d_res.cpu().tolist()]
        pns = [int(x) & U64 for x in self.d_pn.cpu().tolist()]
        assert m <= len(rx)
        assert (sel[m:] == SEL_SENT).all() and res[m:] == [SENTINEL] * (cap - m) and pns[m:] == [SENTINEL] * (cap - m)
        assert (gens[m if not plain else 0:] == GEN_SENT).all()
        self.sel, self.res, self.pns, self.gens = sel[:m].tolist(), res[:m], pns[:m], gens[:m].tolist()
        self.pkt, self.out = d_buf.cpu().numpy(), d_out.cpu().numpy()


def expect(keys, states, stride, buf, pkts, out_total, plain=False):
    """what the model and the plain-Python packet protection make of the descriptors `pkts` over the packet buffer `buf`, from
    the bytes alone: (results, packet numbers, generations, the packet buffer after, the output buffer)"""
    algo = keys.case.algo
    want_pkt, want_out, res, pns, gens = buf.copy(), np.full(out_total, FILL, np.uint8), [], [], []
    for p in pkts:
        o, n, po, c = int(p["pkt_off"]), int(p["pkt_len"]), int(p["pn_offset"]), int(p["key"])
        packet = want_pkt[o: o + n].tobytes()
        masked = not int(p["flags"]) & ptls_hip.QUIC_UNPROTECTED
        mask = quic_ref.hp_mask(algo, keys.hps[int(p["hp_key"])], packet[po + 4: po + 20]) if masked else bytes(16)
        first = packet[0] ^ (mask[0] & quic_ref.first_byte_bits(packet[0]))
        pn_len = (first & 3) + 1
        header = quic_ref.apply_mask(packet[:po + pn_len], po, pn_len, mask)
        pn = quic_ref.decode_pn(int(p["pn"]), int.from_bytes(header[po:], "big"), pn_len)
        g = NO_GEN if plain else model.choose(first, pn, *states[c])
        key, iv = keys.table[model.slot(c, stride, g)]
        pt, ok = quic_ref.aead_open(algo, key, iv, pn, header, packet[po + pn_len:])
        res.append(len(pt) if ok else U64)
        pns.append(pn)
        gens.append(g)
        want_pkt[o: o + len(header)] = np.frombuffer(header, np.uint8)
        want_out[int(p["data_off"]): int(p["data_off"]) + len(pt)] = np.frombuffer(pt, np.uint8)
    return res, pns, gens, want_pkt, want_out


def check(o, keys, states, stride, buf, pkts, want_sel, out_total):
    assert o.sel == list(want_sel)
    res, pns, gens, want_pkt, want_out = expect(keys, states, stride, buf, pkts[list(want_sel)], out_total)
    assert o.gens == gens
    assert o.res == res and o.pns == pns
    assert np.array_equal(o.pkt, want_pkt)
    assert np.array_equal(o.out, want_out)
    return res


def run_case(engine, keys, case, packets=None, unprotected=False):
    """a case's packets through set_packets and one open_keyphase; checked against the reference and the case's own labels"""
    packets = case.packets if packets is None else packets
    buf, pkts, pkt_total, out_total = lay_out(case, packets, unprotected)
    rx = ptls_hip.QuicRx(engine, 0, len(pkts))
    try:
        load(rx, pkts)
        d_phase = dev(phase_table(case.states).view(np.uint8))
        o = Opened(rx, keys, d_phase, case.count, case.stride, dev(buf), pkt_total, out_total)
        res = check(o, keys, case.states, case.stride, buf, pkts, range(len(pkts)), out_total)
        assert o.gens == [p.want_gen for p in packets] and o.pns == [p.pn for p in packets]
        assert res == [len(p.payload) if case.must_open(p) else U64 for p in packets]
        assert read_table(d_phase) == case.states  # the open call only reads the state
        assert o.rep.planned_on_device == 1 and (case.algo == "chacha" or o.rep.lanes == 64)
        return o, buf
    finally:
        torch.cuda.synchronize()
        rx.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_three_banks(engine, keyed, algo):
    """current, next and previous generation packets of 130 connections with gen 0..5, shuffled: all open, each under its bank"""
    case = gen.three_banks(algo)
    o, _ = run_case(engine, keyed(case), case)
    assert U64 not in o.res and {g % 3 for g in o.gens} == {0, 1, 2}


@pytest.mark.parametrize("algo", ALGOS)
def test_one_key_only(engine, keyed, algo):
    """sealed under gen + 2, or under the previous generation on a pn >= first_pn: the one key tried refuses them, and gen_out is
    still the rule's value"""
    case = gen.one_key_only(algo)
    o, _ = run_case(engine, keyed(case), case)
    assert o.res.count(U64) == len(case.packets) - 9


@pytest.mark.parametrize("algo", ["aes128", "chacha"])
def test_the_gap(engine, keyed, algo):
    """the peer's first packets after its key update: through rx.open under the current generation's slot every one fails;
    through open_keyphase they open"""
    case = gen.three_banks(algo)
    nxt = [p for p in case.packets if p.want_gen == case.states[p.conn][0] + 1]
    assert len(nxt) > 80
    keys = keyed(case)
    buf, pkts, pkt_total, out_total = lay_out(case, nxt)
    today = pkts.copy()
    today["key"] = [model.slot(p.conn, case.stride, case.states[p.conn][0]) for p in nxt]
    rx = ptls_hip.QuicRx(engine, 0, len(nxt))
    try:
        load(rx, today)
        old = Opened(rx, keys, None, 0, 0, dev(buf), pkt_total, out_total, plain=True)
        assert old.sel == list(range(len(nxt))) and old.res == [U64] * len(nxt) and old.pns == [p.pn for p in nxt]
        load(rx, pkts)
        d_phase = dev(phase_table(case.states).view(np.uint8))
        new = Opened(rx, keys, d_phase, case.count, case.stride, dev(buf), pkt_total, out_total)
        assert check(new, keys, case.states, case.stride, buf, pkts, range(len(nxt)), out_total) == [len(p.payload) for p in nxt]
    finally:
        torch.cuda.synchronize()
        rx.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_long_headers_and_the_unprotected_flag(engine, keyed, algo):
    """Handshake packets whose unmasked first byte has 0x04 set, between 1-RTT packets in one call: their key is unchanged and
    gen_out is NO_GEN.  Then the same packets with their headers already unprotected and PTLS_HIP_QUIC_UNPROTECTED: the bit is
    taken as it stands and no byte of the packet buffer changes"""
    case = gen.long_and_short(algo)
    keys = keyed(case, hp_slots=40)
    assert sum(1 for p in case.packets if p.long and p.header[0] & 4) >= 12
    o, _ = run_case(engine, keys, case)
    assert [g == NO_GEN for g in o.gens] == [p.long for p in case.packets] and U64 not in o.res
    f, buf = run_case(engine, keys, case, unprotected=True)
    assert np.array_equal(f.pkt, buf) and f.gens == o.gens and f.res == o.res and np.array_equal(f.out, o.out)


@pytest.mark.parametrize("stride,count", [(10, 14), (14, 10), (12, 12)])
def test_select_bound(engine, keyed, stride, count):
    """key at stride - 1, stride, count - 1 and count (and 0, and no connection) over random bytes: selected if and only if
    key < min(stride, count), as the model says; every selected packet fails and is written as the reference says"""
    case = gen.Case("chacha", [[c % 4, 50] for c in range(count)], stride, [], gen.NCONN)
    keys = keyed(case, hp_slots=16)
    want_keys = [0, stride - 1, stride, count - 1, count, ptls_hip.QUIC_NO_CONN, min(stride, count) - 1, min(stride, count), 3 * stride - 1, 1]
    n = len(want_keys)
    pkts = np.zeros(n, dtype=ptls_hip.QUIC_PACKET_DTYPE)
    pkts["pkt_off"], pkts["data_off"] = 1 + 128 * np.arange(n), 128 * np.arange(n)
    pkts["pkt_len"], pkts["pn_offset"], pkts["key"], pkts["hp_key"], pkts["pn"] = 60 + np.arange(n), 9, want_keys, np.arange(n), 40
    total = 128 * n + 64
    buf = np.random.default_rng(stride).integers(0, 256, total, dtype=np.uint8)
    want_sel = quic_rx_ref.select(pkts, None, total, total, model.limit(stride, count), 16)
    assert want_sel == [j for j, k in enumerate(want_keys) if k < min(stride, count)] and 3 < len(want_sel) < n - 3
    rx = ptls_hip.QuicRx(engine, 0, n)
    try:
        load(rx, pkts)
        o = Opened(rx, keys, dev(phase_table(case.states).view(np.uint8)), count, stride, dev(buf), total, total)
        assert check(o, keys, case.states, stride, buf, pkts, want_sel, total) == [U64] * len(want_sel)
    finally:
        torch.cuda.synchronize()
        rx.close()


def test_refusals(engine, keyed):
    """every refusal of rx_open_keyphase, with real keysets: nothing launched, nothing written; and the commit's, which needs
    an rx_open_keyphase in front of it"""
    case = gen.one_key_only("aes128")
    keys = keyed(case)
    buf, pkts, pkt_total, out_total = lay_out(case)
    rx = ptls_hip.QuicRx(engine, 0, len(pkts))
    L = ptls_hip.lib()
    try:
        load(rx, pkts)
        d_buf, d_phase = dev(buf), dev(phase_table(case.states).view(np.uint8))
        cap = len(pkts) + 8
        d_out = torch.full((out_total,), FILL, dtype=torch.uint8, device="cuda")
        d_sel, d_gen = u32(np.full(cap, SEL_SENT)), u32(np.full(cap, GEN_SENT))
        d_res = torch.full((cap,), SENTINEL, dtype=torch.int64, device="cuda")
        d_pn = torch.full((cap,), SENTINEL, dtype=torch.int64, device="cuda")
        rep = ptls_hip.QuicRxReport(9, 9, 9)

        def call(phase=d_phase.data_ptr(), count=case.count, stride=case.stride, g=d_gen.data_ptr(), null_kp=False, b=d_buf.data_ptr()):
            kp = ptls_hip.QuicRxKeyphase(phase, count, stride, g)
            return L.ptls_hip_quic_rx_open_keyphase(rx.ptr, keys.ks.ptr, keys.hp.ptr, ALL, None if null_kp else ctypes.addressof(kp), b,
                                                    pkt_total, d_out.data_ptr(), out_total, d_sel.data_ptr(), d_res.data_ptr(),
                                                    d_pn.data_ptr(), ctypes.addressof(rep), None)

        third = (1 << 64) // 3
        for kw, msg in ((dict(null_kp=True), "null key-phase parameters"), (dict(phase=None), "null key-phase state"),
                        (dict(g=None), "null key-phase state or generation array"), (dict(stride=0), "stride or a state count of 0"),
                        (dict(count=0), "stride or a state count of 0"),
                        (dict(stride=case.stride + 1), "three banks of stride 138 do not fit the keyset's 411 slots"),
                        (dict(stride=third + 1), "do not fit the keyset's 411 slots"),  # 3 * stride wraps to 2
                        (dict(stride=third + 46), "do not fit the keyset's 411 slots"),  # ... to 137
                        (dict(stride=1 << 63), "do not fit"), (dict(stride=(1 << 64) - 1), "do not fit")):
            assert call(**kw) == ptls_hip.EINVAL, kw
            assert "quic_rx_open_keyphase:" in ptls_hip.last_error() and msg in ptls_hip.last_error(), (kw, ptls_hip.last_error())
        rx.set_plan(ptls_hip.QUIC_RX_PLAN_HOST)
        assert call() == ptls_hip.EINVAL and "fixes a chunk's key on the host" in ptls_hip.last_error()
        rx.set_plan(ptls_hip.QUIC_RX_PLAN_AUTO)
        assert (rep.n_selected, rep.planned_on_device, rep.lanes) == (9, 9, 9)
        assert call(b=None) == ptls_hip.EINVAL and "quic_rx_open_keyphase: null buffer" in ptls_hip.last_error()  # rx_open's own, as there
        d_upd = u32(np.full(case.count + 8, SEL_SENT))
        with pytest.raises(ptls_hip.HipError, match="no rx_open_keyphase on the object"):
            rx.keyphase_commit(d_phase, case.count, d_res, d_pn, d_gen, d_upd)
        torch.cuda.synchronize()
        assert (d_out == FILL).all() and (d_res == SENTINEL).all() and (d_pn == SENTINEL).all()
        assert (d_sel.cpu().numpy().view(np.uint32) == SEL_SENT).all() and (d_gen.cpu().numpy().view(np.uint32) == GEN_SENT).all()
        assert np.array_equal(d_buf.cpu().numpy(), buf) and read_table(d_phase) == case.states
        # the largest stride the keyset takes is not refused; a plain open in between takes the commit's packets away
        assert call(stride=case.stride) == 0 and rep.n_selected == len(pkts)
        torch.cuda.synchronize()
        Opened(rx, keys, None, 0, 0, dev(buf), pkt_total, out_total, plain=True)
        with pytest.raises(ptls_hip.HipError, match="no rx_open_keyphase on the object"):
            rx.keyphase_commit(d_phase, case.count, d_res, d_pn, d_gen, d_upd)
        assert (d_upd.cpu().numpy().view(np.uint32) == SEL_SENT).all()
    finally:
        torch.cuda.synchronize()
        rx.close()


def test_forced_device_plan_on_one_key(engine, keysets):
    """the one-key shape of test_gpu_quic_rx.test_fallback_on_one_key, AES: rx_open plans it on the host for the batch kernel;
    open_keyphase takes the wave-per-record kernel whatever the key runs say, and the bytes are the same"""
    algo = "aes128"
    ks, hp = keysets(algo)
    sp = [s for s in specs("one") if len(s.payload) == 1200][:1] * 64
    buf, pkts, pkt_total, out_total = spec_input(algo, sp, protected(algo, sp))
    stride = NKEYS // 3
    g = 3 if sp[0].header[0] & 4 else 0  # bank 0 holds the generation of the packets' bit: the slot is the packets' own
    states = [[g, 0]]

    class K:  # the module-wide keysets of test_gpu_quic as a case's keys
        case = gen.Case(algo, states, stride, [], 1)
        hps = key_material(algo)[2]
        table = dict(enumerate(zip(*key_material(algo)[:2])))
    K.ks, K.hp = ks, hp
    assert sp[0].slot == 0
    rx = ptls_hip.QuicRx(engine, 0, 64)
    try:
        load(rx, pkts)
        old = Opened(rx, K, None, 0, 0, dev(buf), pkt_total, out_total, plain=True)
        assert old.rep.planned_on_device == 0 and old.rep.lanes != 64 and old.res == [1200] * 64
        new = Opened(rx, K, dev(phase_table(states).view(np.uint8)), 1, stride, dev(buf), pkt_total, out_total)
        assert (new.rep.planned_on_device, new.rep.lanes) == (1, 64)
        assert check(new, K, states, stride, buf, pkts, range(64), out_total) == [1200] * 64
        assert new.gens == [g] * 64 and np.array_equal(new.out, old.out) and np.array_equal(new.pkt, old.pkt)
    finally:
        torch.cuda.synchronize()
        rx.close()


@pytest.mark.parametrize("algo", ["aes128", "chacha"])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_header_kernel_sizes(engine, keyed, algo, n):
    case = gen.three_banks(algo)
    assert len(case.packets) >= 257
    run_case(engine, keyed(case), case, case.packets[:n])


def commit(rx, o, d_phase, count):
    """rx.keyphase_commit over an Opened's arrays: (the updated connections, the table after)"""
    d_upd = u32(np.full(count + 8, SEL_SENT))
    n = rx.keyphase_commit(d_phase, count, o.d_res, o.d_pn, o.d_gen, d_upd)
    torch.cuda.synchronize()
    upd = d_upd.cpu().numpy().view(np.uint32)
    assert n <= count and (upd[n:] == SEL_SENT).all()
    return upd[:n].tolist(), read_table(d_phase)


@pytest.mark.parametrize("algo", ALGOS)
def test_commit_then_open_again(engine, keyed, algo):
    """open, commit, re-key the freed banks, open fresh packets: the table and the list of updated connections are the
    model's; a connection whose only next-generation packets are damaged does not advance; a reordered current-generation
    packet lowers first_pn; the second open chooses by the state the device left"""
    case = gen.commit_case(algo)
    keys = keyed(case)
    buf, pkts, pkt_total, out_total = lay_out(case)
    want = [list(s) for s in case.states]
    want_upd = model.commit(want, *gen.commit_inputs(case))
    stuck = [c for c in range(case.count) if c % 7 == 3 and any(p.damaged for p in case.packets if p.conn == c)]
    lowered = [c for c in range(case.count) if want[c][0] == case.states[c][0] and want[c][1] < case.states[c][1]]
    assert len(want_upd) > 60 and len(stuck) > 8 and not set(stuck) & set(want_upd) and len(lowered) > 10
    assert all(want[c] == [case.states[c][0] + 1, min(p.pn for p in case.packets if p.conn == c and p.want_gen == want[c][0])]
               for c in want_upd)
    rx = ptls_hip.QuicRx(engine, 0, len(pkts))
    try:
        load(rx, pkts)
        d_phase = dev(phase_table(case.states).view(np.uint8))
        o = Opened(rx, keys, d_phase, case.count, case.stride, dev(buf), pkt_total, out_total)
        res = check(o, keys, case.states, case.stride, buf, pkts, range(len(pkts)), out_total)
        assert (gen.commit_inputs(case)[1], gen.commit_inputs(case)[3]) == (res, o.gens)
        upd, table = commit(rx, o, d_phase, case.count)
        assert upd == want_upd and table == want
        # a second commit over the same arrays: the updated connections' packets are now of the current generation
        again = [list(s) for s in want]
        assert model.commit(again, *gen.commit_inputs(case)) == [] and commit(rx, o, d_phase, case.count) == ([], again)
        # the host re-keys: for an updated connection the bank of the old previous generation now holds gen + 2's keys
        after = gen.after_commit(algo, again)
        keys.set_banks(after)
        c = want_upd[0]
        assert keys.table[model.slot(c, case.stride, again[c][0] + 1)] == case.keys[c][case.states[c][0] + 2]
        buf2, pkts2, pkt_total2, out_total2 = lay_out(after)
        rx2 = ptls_hip.QuicRx(engine, 0, len(pkts2))
        try:
            load(rx2, pkts2)
            o2 = Opened(rx2, keys, d_phase, case.count, case.stride, dev(buf2), pkt_total2, out_total2)  # the device's table
            assert check(o2, keys, again, case.stride, buf2, pkts2, range(len(pkts2)), out_total2) == [len(p.payload) for p in after.packets]
            assert o2.gens == [p.want_gen for p in after.packets]
        finally:
            torch.cuda.synchronize()
            rx2.close()
    finally:
        torch.cuda.synchronize()
        rx.close()


def test_commit_scratch_grows(engine, keyed):
    """one receive object, one open_keyphase over 12 packets of 5 connections, then a commit with count = 2 and one with
    count = 5: the minima and the scan levels grow between the two.  Connections 1 and 4 send next-generation packets: the first
    commit finds connection 1's update and leaves entries 2 .. 4 alone, the second finds connection 4's and lowers first_pn
    of 2 and 3.  Both lists and the table are the model's, applied in the same two steps; a third commit finds nothing left"""
    states = [[c % 2, 100] for c in range(5)]
    pk = [gen.short_packet(c, g, 120 + c, 8 + c % 2) for c, (g, _) in enumerate(states)]
    pk += [gen.short_packet(c, states[c][0] + 1, 130 + c, 8) for c in (4, 1)]
    pk += [gen.short_packet(c, g, 95 - c, 9) for c, (g, _) in enumerate(states)]  # reordered: below first_pn
    case = gen.Case("aes128", states, 6, pk, gen.NCONN)
    assert len(pk) == 12 and all(case.must_open(p) for p in pk)
    keys = keyed(case)
    buf, pkts, pkt_total, out_total = lay_out(case)
    conns, res, pns, gens = gen.commit_inputs(case)
    head = [list(s) for s in states[:2]]
    first_upd = model.commit(head, conns, res, pns, gens)
    after_first = head + [list(s) for s in states[2:]]
    want = [list(s) for s in after_first]
    second_upd = model.commit(want, conns, res, pns, gens)
    assert (first_upd, second_upd) == ([1], [4]) and after_first[1] == [2, 131] and want[2:] == [[0, 93], [1, 92], [1, 134]]
    rx = ptls_hip.QuicRx(engine, 0, len(pkts))
    try:
        load(rx, pkts)
        d_phase = dev(phase_table(states).view(np.uint8))
        o = Opened(rx, keys, d_phase, case.count, case.stride, dev(buf), pkt_total, out_total)
        assert check(o, keys, states, case.stride, buf, pkts, range(len(pkts)), out_total) == res
        assert (o.pns, o.gens) == (pns, gens)
        assert commit(rx, o, d_phase, 2) == (first_upd, after_first)
        assert commit(rx, o, d_phase, 5) == (second_upd, want)
        again = [list(s) for s in want]
        assert model.commit(again, conns, res, pns, gens) == [] and commit(rx, o, d_phase, 5) == ([], again)
    finally:
        torch.cuda.synchronize()
        rx.close()


def test_commit_groupings_of_bulk_traffic(engine, keyed):
    """1 500 packets of four connections in buffer order, laid out so that the mark pass folds a lane's successive packets,
    flushes when the place changes, reduces waves that hold one place (with the lowest packet number in lanes 37 and 13 of
    later waves, and with lanes that hold nothing) and meets waves that hold two places: the table equals the model's, so
    every minimum came through its grouping"""
    case = gen.grouping_case("aes128")
    paths = gen.mark_paths(case)
    assert paths["fold"] > 500 and paths["flush"] > 100 and paths["reduce"] >= 4 and paths["partial"] >= 2 and paths["split"] >= 2
    assert {13, 37} <= paths["low_lanes"]
    keys = keyed(case)
    buf, pkts, pkt_total, out_total = lay_out(case)
    conns, res, pns, gens = gen.commit_inputs(case)
    want = [list(s) for s in case.states]
    want_upd = model.commit(want, conns, res, pns, gens)
    assert want_upd == [1, 3] and want == [[2, 7], [2, 150], [4, 7594], [4, 7593]]  # (forged packets carry 3: never taken)
    rx = ptls_hip.QuicRx(engine, 0, len(pkts))
    try:
        load(rx, pkts)
        d_phase = dev(phase_table(case.states).view(np.uint8))
        o = Opened(rx, keys, d_phase, case.count, case.stride, dev(buf), pkt_total, out_total)
        assert check(o, keys, case.states, case.stride, buf, pkts, range(len(pkts)), out_total) == res
        assert (o.pns, o.gens) == (pns, gens)
        assert commit(rx, o, d_phase, case.count) == (want_upd, want)
        # again from the state this left: connections 1 and 3 now count their packets as current ones, lowest numbers kept
        assert commit(rx, o, d_phase, case.count) == ([], want)
        # and from a state whose first_pn lies above every number: each current-generation minimum is found again
        high = [[g, 10 ** 7] for g, _ in want]
        want_high = [list(s) for s in high]
        assert model.commit(want_high, conns, res, pns, gens) == [] and want_high == want
        d_high = dev(phase_table(high).view(np.uint8))
        assert commit(rx, o, d_high, case.count) == ([], want_high)
    finally:
        torch.cuda.synchronize()
        rx.close()


@pytest.mark.parametrize("count", [2047, 2048, 2049])
def test_commit_scan_seam(engine, keyed, count):
    """one packet per connection around one scan span, scattered updates (the last connections among them), damaged updates
    and lowered first_pn: results, generations, the table and the ascending list against the model"""
    case = gen.seam_case("aes128", count)
    keys = keyed(case)
    buf, pkts, pkt_total, out_total = lay_out(case)
    conns, res, pns, gens = gen.commit_inputs(case)
    want = [list(s) for s in case.states]
    want_upd = model.commit(want, conns, res, pns, gens)
    assert count - 1 in want_upd and 400 < len(want_upd) < 450 and sum(a[1] < 100 for a in want) > 300
    rx = ptls_hip.QuicRx(engine, 0, len(pkts))
    try:
        load(rx, pkts)
        d_phase = dev(phase_table(case.states).view(np.uint8))
        o = Opened(rx, keys, d_phase, case.count, case.stride, dev(buf), pkt_total, out_total)
        assert o.sel == list(range(count)) and (o.res, o.pns, o.gens) == (res, pns, gens)
        assert commit(rx, o, d_phase, count) == (want_upd, want)
        # a smaller table than the open's: connections outside it are left alone, inside it nothing is left to do
        assert commit(rx, o, d_phase, 100) == ([], want)
    finally:
        torch.cuda.synchronize()
        rx.close()
