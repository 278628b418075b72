"""The receive object on the GPU (include/ptls_hip.h 2i; hsig-picotls_amd/csrc/quic_rx.cpp, quic_rx_kernel.hip): parsed entries
that stay on the device, selected, packed, planned and opened there.  Bit-exact, no tolerance anywhere: the selection against
the plain-Python model (tests/quic_rx_ref.py), every result, packet number, the whole packet buffer and the whole 0xA5-filled
output buffer against the plain-Python packet protection (tests/quic_ref.py) and, byte for byte, against what the existing
parse -> QuicBatch(open) path gives for the same input.  d_sel, d_result and d_pn_out start sentinel-filled with 8 elements to
spare, and what lies behind n_selected must come back untouched.

Sizes: the select / compact scan's seams are QP_SCAN_SPAN = 2048 entries; the sort's tile is QRX_TILE = 1024 positions, and its
[digit][tile] count array (64 per tile) needs a second scan level from 32 tiles + 1 position on."""
import ctypes
import random

import numpy as np
import pytest
import torch

import ptls_hip
import quic_parse_cases as gen
import quic_parse_ref as ref
import quic_ref
import quic_rx_ref as model
from test_gpu_quic import (ALGO_OF, FILL, NKEYS, SENTINEL, U64, descriptors, dev, flip, image, key_material, keysets,  # noqa: F401
                           place, protected, specs)
from test_gpu_quic_parse import E2E_CIDS, NCONN, e2e_packet, lay_out, open_parsed, reference

pytestmark = pytest.mark.gpu
SEL_SENT = 0xC3C3C3C3
ALL = ptls_hip.QUIC_ALL_TYPES


def i64(values):
    return torch.tensor(np.array(values, dtype=np.uint64).view(np.int64), device="cuda")


class Opened:
    """one rx.open() with fresh sentinel-filled arrays: everything read back"""

    def __init__(self, rx, ks, hp, d_buf, buf_len, out_total, mask=ALL, out_len=None):
        cap = len(rx) + 8
        d_out = torch.full((out_total,), FILL, dtype=torch.uint8, device="cuda")
        d_sel = torch.from_numpy(np.full(cap, SEL_SENT, np.uint32).view(np.int32)).cuda()
        d_res = torch.full((cap,), SENTINEL, dtype=torch.int64, device="cuda")
        d_pn = torch.full((cap,), SENTINEL, dtype=torch.int64, device="cuda")
        self.rep = rx.open(ks, hp, d_buf, buf_len, d_out, out_total if out_len is None else out_len, d_sel, d_res, d_pn, type_mask=mask)
        torch.cuda.synchronize()
        self.m = m = int(self.rep.n_selected)
        sel = d_sel.cpu().numpy().view(np.uint32)
        res = [int(x) & U64 for x in d_res.cpu().tolist()]
        pns = [int(x) & U64 for x in d_pn.cpu().tolist()]
        assert m <= len(rx)
        assert (sel[m:] == SEL_SENT).all() and res[m:] == [SENTINEL] * (cap - m) and pns[m:] == [SENTINEL] * (cap - m)
        self.sel, self.res, self.pns = sel[:m].tolist(), res[:m], pns[:m]
        self.pkt, self.out = d_buf.cpu().numpy(), d_out.cpu().numpy()
        self.order = rx.order(m)

    def same_outputs(self, other):
        return (self.sel == other.sel and self.res == other.res and self.pns == other.pns and np.array_equal(self.pkt, other.pkt)
                and np.array_equal(self.out, other.out))


def expect(algo, buf, pkts, out_total):
    """what the plain-Python packet protection makes of the descriptors `pkts` over the packet buffer `buf`:
    (results, packet numbers, the packet buffer after, the output buffer)"""
    keys, ivs, hps = key_material(algo)
    want_pkt, want_out, res, pns = buf.copy(), np.full(out_total, FILL, np.uint8), [], []
    for p in pkts:
        o, n, po = int(p["pkt_off"]), int(p["pkt_len"]), int(p["pn_offset"])
        header, pn, pt, ok = quic_ref.unprotect(algo, keys[int(p["key"])], ivs[int(p["key"])], hps[int(p["hp_key"])],
                                                want_pkt[o: o + n].tobytes(), po, int(p["pn"]),
                                                protected=not int(p["flags"]) & ptls_hip.QUIC_UNPROTECTED)
        res.append(len(pt) if ok else U64)
        pns.append(pn)
        want_pkt[o: o + len(header)] = np.frombuffer(header, np.uint8)
        want_out[int(p["data_off"]): int(p["data_off"]) + len(pt)] = np.frombuffer(pt, np.uint8)
    return res, pns, want_pkt, want_out


def check(o, algo, buf, pkts, want_sel, out_total):
    """an Opened against the model's selection and the reference's bytes"""
    assert o.sel == list(want_sel)
    res, pns, want_pkt, want_out = expect(algo, buf, pkts[list(want_sel)], out_total)
    assert o.res == res and o.pns == pns
    assert np.array_equal(o.pkt, want_pkt)
    assert np.array_equal(o.out, want_out)
    return res


def load(rx, pkts, info=None):
    d_pkts = torch.from_numpy(np.ascontiguousarray(pkts).view(np.uint8)).cuda()
    d_info = torch.from_numpy(np.ascontiguousarray(info).view(np.uint8)).cuda() if info is not None else None
    rx.set_packets(d_pkts, d_info, len(pkts))
    torch.cuda.synchronize()
    assert len(rx) == len(pkts)


def e2e_input(algo):
    """the 40 datagrams of test_gpu_quic_parse.test_end_to_end_parse_then_open: coalesced packets of 12 connections, an unknown
    connection, a Retry: (buffer, datagram array, expected packet numbers, the model's connection-ID map)"""
    rng = random.Random(ALGO_OF[algo][1] + len(algo))
    base = [[(1 << 33) + 1000 * c, 50 + c, (1 << 20) * c + 7] for c in range(NCONN)]
    cases = []
    for i in range(40):
        conn = i % NCONN
        kinds = [(ref.HANDSHAKE, ref.ONE_RTT), (ref.ONE_RTT,), (ref.ZERO_RTT, ref.HANDSHAKE, ref.ONE_RTT), (ref.INITIAL, ref.HANDSHAKE)][i % 4]
        d = b"".join(e2e_packet(rng, algo, conn, k, base[conn][ref.pn_space(k)])[0] for k in kinds)
        if i % 10 == 3:
            d = gen.long_packet(rng, ref.V1, ref.HANDSHAKE, b"\xEE" * 8, b"")[0] + d
        if i % 20 == 7:
            d = d + gen.long_packet(rng, ref.V1, ref.RETRY, E2E_CIDS[0], b"")[0]
        cases.append((d, b""))
    buf, dg = lay_out(cases, 21)
    cmodel = ref.CidMap(NCONN)
    for c, cid in enumerate(E2E_CIDS):
        cmodel.set(cid, c)
    return buf, dg, [v for row in base for v in row], cmodel


def parse_into(engine, rx, buf, dg, flat, d_buf):
    m = ptls_hip.QuicCidMap(engine, NCONN)
    try:
        m.set(E2E_CIDS, list(range(NCONN)))
        n = rx.parse(dg, d_buf, len(buf), cidmap=m, short_cid_len=8, expected_pn=i64(flat))
        torch.cuda.synchronize()
    finally:
        m.close()
    return n


@pytest.mark.parametrize("algo", ["aes128", "aes256", "chacha"])
def test_end_to_end(engine, keysets, algo):
    ks, hp = keysets(algo)
    buf, dg, flat, cmodel = e2e_input(algo)
    want_pkts, want_info = reference(buf, dg, short_cid_len=8, cidmap=cmodel, expected_pn=flat)
    total = len(buf)
    rx = ptls_hip.QuicRx(engine, len(dg), len(want_pkts) + 3)
    try:
        d_buf = dev(buf)
        assert parse_into(engine, rx, buf, dg, flat, d_buf) == len(want_pkts) == len(rx)
        assert np.array_equal(rx.packets(), want_pkts) and np.array_equal(rx.info(), want_info)
        want_sel = model.select(want_pkts, want_info, total, total, NKEYS, NKEYS)
        assert len(want_sel) == len(want_pkts) - 6
        o = Opened(rx, ks, hp, d_buf, total, total)
        res = check(o, algo, buf, want_pkts, want_sel, total)
        assert U64 not in res and o.rep.planned_on_device == 1
        # byte for byte what the existing path gives
        old = open_parsed(engine, ks, hp, np.ascontiguousarray(want_pkts[want_sel]), dev(buf), total)
        assert (o.res, o.pns) == old[:2] and np.array_equal(o.pkt, old[2]) and np.array_equal(o.out, old[3])
        # the host plan and the device plan: identical outputs everywhere
        runs = {}
        for mode in (ptls_hip.QUIC_RX_PLAN_DEVICE, ptls_hip.QUIC_RX_PLAN_HOST):
            rx.set_plan(mode)
            runs[mode] = Opened(rx, ks, hp, dev(buf), total, total)
            assert runs[mode].rep.planned_on_device == (1 if mode == ptls_hip.QUIC_RX_PLAN_DEVICE else 0)
            assert runs[mode].same_outputs(o)
        if algo != "chacha":
            sel_pkts = want_pkts[want_sel]
            assert np.array_equal(runs[ptls_hip.QUIC_RX_PLAN_DEVICE].order, model.plan_order(sel_pkts))
            assert runs[ptls_hip.QUIC_RX_PLAN_HOST].order is None
        # too small an object: the count comes back, nothing is loaded
        small = ptls_hip.QuicRx(engine, len(dg), len(want_pkts) - 1)
        try:
            with pytest.raises(ptls_hip.HipError, match="%d entries do not fit the receive object's %d" % (len(want_pkts), len(want_pkts) - 1)):
                parse_into(engine, small, buf, dg, flat, d_buf)
            assert len(small) == 0
        finally:
            small.close()
    finally:
        torch.cuda.synchronize()
        rx.close()


@pytest.mark.parametrize("algo", ["aes128", "chacha"])
def test_type_masks(engine, keysets, algo):
    """one parse, then 1-RTT only, then Handshake only, into separate arrays; the second open sees the headers the first left
    protected, and the buffer the first left behind"""
    ks, hp = keysets(algo)
    buf, dg, flat, cmodel = e2e_input(algo)
    pkts, info = reference(buf, dg, short_cid_len=8, cidmap=cmodel, expected_pn=flat)
    total = len(buf)
    rx = ptls_hip.QuicRx(engine, 64, 256)
    try:
        d_buf = dev(buf)
        parse_into(engine, rx, buf, dg, flat, d_buf)
        after = buf
        for mask in (1 << ref.ONE_RTT, 1 << ref.HANDSHAKE, 0, 1 << ref.RETRY):
            want_sel = model.select(pkts, info, total, total, NKEYS, NKEYS, mask)
            assert (len(want_sel) > 20) == (mask in (1 << ref.ONE_RTT, 1 << ref.HANDSHAKE))
            assert all(1 << int(info["type"][k]) == mask for k in want_sel)
            o = Opened(rx, ks, hp, d_buf, total, total, mask=mask)
            check(o, algo, after, pkts, want_sel, total)
            after = o.pkt
    finally:
        torch.cuda.synchronize()
        rx.close()


def boundary_descriptors(buf_len, out_len):
    """hand-made descriptors, one boundary of the select rule each, in slots of 512 bytes; the ones that sit at the buffers'
    ends come last: (descriptors, types)"""
    rows = []

    def add(**kw):
        k = len(rows)
        d = dict(pkt_off=512 * k + 1, data_off=512 * k + 3, pkt_len=120, key=k % NKEYS, hp_key=(k * 5 + 1) % NKEYS, pn_offset=9, pn=k, type=k % 8)
        d.update(kw)
        rows.append(d)

    for k in range(8):
        add()
    add(pn_offset=0)
    add(pkt_len=9 + 19)
    add(pkt_len=9 + 20)
    add(pn_offset=47, pkt_len=47 + 19)
    add(pn_offset=47, pkt_len=47 + 20)
    add(pkt_len=65535, pkt_off=2, data_off=0)
    add(pkt_len=65536, pkt_off=2, data_off=0)
    add(pkt_len=0xFFFFFFFF)
    for v in (NKEYS - 1, NKEYS, ptls_hip.QUIC_NO_CONN):
        add(key=v)
        add(hp_key=v)
    for d in (-1, 0, 1):
        add(pkt_off=buf_len - 120 + d)                    # ends at buf_len - 1 / buf_len / buf_len + 1
        add(data_off=out_len - (120 - 9 - 17) + d)        # the area ends at out_len - 1 / out_len / out_len + 1
    add(pkt_off=(1 << 64) - 60)
    add(data_off=(1 << 64) - 50)
    for k in range(5):
        add()
    p = np.zeros(len(rows), dtype=ptls_hip.QUIC_PACKET_DTYPE)
    for f in ("pkt_off", "data_off", "pkt_len", "key", "hp_key", "pn_offset", "pn"):
        p[f] = np.array([r[f] for r in rows], dtype=np.uint64).astype(p.dtype[f])
    info = np.zeros(len(rows), dtype=ptls_hip.QUIC_PKTINFO_DTYPE)
    info["type"] = [r["type"] for r in rows]
    return p, info


@pytest.mark.parametrize("algo", ["aes128", "chacha"])
@pytest.mark.parametrize("with_info,mask", [(False, 0), (True, 0x15), (True, ALL)])
def test_device_side_refusals(engine, keysets, algo, with_info, mask):
    """descriptors through rx_set_packets over random bytes: d_sel equals the model; outside the header bytes of selected
    packets and outside their plaintext areas nothing changes, and buf_len / out_len are the limits even though the
    allocations go on behind them"""
    ks, hp = keysets(algo)
    buf_len = out_len = 70000
    rng = np.random.default_rng(3)
    buf = rng.integers(0, 256, buf_len + 256, dtype=np.uint8)
    pkts, info = boundary_descriptors(buf_len, out_len)
    want_sel = model.select(pkts, info if with_info else None, buf_len, out_len, NKEYS, NKEYS, mask)
    every = model.select(pkts, None, buf_len, out_len, NKEYS, NKEYS)
    assert len(every) == 8 + 2 + 1 + 2 + 2 * 2 + 5 and (len(want_sel) < len(every)) == (mask == 0x15)
    rx = ptls_hip.QuicRx(engine, 0, len(pkts))
    try:
        load(rx, pkts, info if with_info else None)
        assert np.array_equal(rx.packets(), pkts) and (rx.info() is None) == (not with_info)
        o = Opened(rx, ks, hp, dev(buf), buf_len, out_len + 256, mask=mask, out_len=out_len)
        assert o.sel == want_sel and o.rep.planned_on_device == 1
        may_pkt, may_out = np.zeros(len(buf), bool), np.zeros(out_len + 256, bool)
        for k in want_sel:
            o_, po = int(pkts["pkt_off"][k]), int(pkts["pn_offset"][k])
            may_pkt[o_] = True
            may_pkt[o_ + po: o_ + po + 4] = True
            may_out[int(pkts["data_off"][k]): int(pkts["data_off"][k]) + int(pkts["pkt_len"][k]) - po - 17] = True
        assert not may_pkt[buf_len:].any() and not may_out[out_len:].any()
        assert np.array_equal(o.pkt[~may_pkt], buf[~may_pkt])
        assert (o.out[~may_out] == FILL).all()
        assert (o.out[may_out] != FILL).any()
    finally:
        torch.cuda.synchronize()
        rx.close()


def spec_input(algo, sp, packets, flags=0, slots=None):
    pkt_offs, pkt_total = place([s.pkt_len for s in sp])
    out_offs, out_total = place([len(s.payload) + 4 for s in sp])
    return image(pkt_total, pkt_offs, packets), descriptors(sp, pkt_offs, out_offs, True, flags, slots), pkt_total, out_total


@pytest.mark.parametrize("algo", ["aes128", "aes256", "chacha"])
def test_damaged_packets(engine, keysets, algo):
    """a flipped ciphertext bit, a flipped tag bit and a first-byte bit that changes pn_len, among intact packets: UINT64_MAX,
    the plaintext written, the reference's bytes"""
    ks, hp = keysets(algo)
    sp = [s for s in specs("many") if len(s.payload) >= 15][::2]
    packets = protected(algo, sp)
    hit = {5: lambda s: (len(s.header) + 7, 3), 40: lambda s: (s.pkt_len - 1, 7), 41: lambda s: (0, 0), 60: lambda s: (0, 1)}
    for j, where in hit.items():
        packets[j] = flip(packets[j], *where(sp[j]))
    buf, pkts, pkt_total, out_total = spec_input(algo, sp, packets)
    rx = ptls_hip.QuicRx(engine, 0, len(pkts))
    try:
        load(rx, pkts)
        o = Opened(rx, ks, hp, dev(buf), pkt_total, out_total)
        res = check(o, algo, buf, pkts, range(len(pkts)), out_total)
        assert [j for j, r in enumerate(res) if r == U64] == sorted(hit) and o.rep.planned_on_device == 1
    finally:
        torch.cuda.synchronize()
        rx.close()


@pytest.mark.parametrize("algo", ["aes128", "chacha"])
@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_scan_seams_of_select_and_compact(engine, keysets, algo, n):
    """n entries around one scan span, every third one unselectable (in turn: no connection, pn_offset 0, too short)"""
    ks, hp = keysets(algo)
    rng = np.random.default_rng(n)
    pkts = np.zeros(n, dtype=ptls_hip.QUIC_PACKET_DTYPE)
    pkts["pkt_len"] = 21 + np.arange(n) % 40
    pkts["pkt_off"] = 1 + 64 * np.arange(n)
    pkts["data_off"] = 64 * np.arange(n)
    pkts["pn_offset"], pkts["key"], pkts["hp_key"] = 1, np.arange(n) % NKEYS, (np.arange(n) * 7) % NKEYS
    bad = np.arange(n) % 3 == 1
    pkts["key"][bad & (np.arange(n) % 9 == 1)] = ptls_hip.QUIC_NO_CONN
    pkts["pn_offset"][bad & (np.arange(n) % 9 == 4)] = 0
    pkts["pkt_len"][bad & (np.arange(n) % 9 == 7)] = 20
    total = 64 * n + 64
    buf = rng.integers(0, 256, total, dtype=np.uint8)
    want_sel = model.select(pkts, None, total, total, NKEYS, NKEYS)
    assert want_sel == [k for k in range(n) if not bad[k]]
    rx = ptls_hip.QuicRx(engine, 0, n)
    try:
        load(rx, pkts)
        o = Opened(rx, ks, hp, dev(buf), total, total)
        assert o.sel == want_sel and o.res == [U64] * len(want_sel) and o.rep.planned_on_device == 1
        if algo != "chacha":
            assert np.array_equal(o.order, model.plan_order(pkts[want_sel]))
    finally:
        torch.cuda.synchronize()
        rx.close()


@pytest.mark.parametrize("m", [model.QRX_TILE - 1, model.QRX_TILE, model.QRX_TILE + 1, model.second_level_m()])
def test_plan_order(engine, keysets, m):
    """AES, the device plan forced and automatic: packets of 21 - 400 bytes whose provisional lengths sit on the 16-byte block
    boundaries, many ties, over random bytes (every result is UINT64_MAX).  rx_order equals the model's stable order, and
    every output equals the forced host plan's"""
    ks, hp = keysets("aes128")
    rng = np.random.default_rng(m)
    pkts = np.zeros(m, dtype=ptls_hip.QUIC_PACKET_DTYPE)
    length = rng.choice(np.array([3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 127, 128, 255, 256, 257, 382]), m)
    pkts["pn_offset"] = 1
    pkts["pkt_len"] = 18 + length
    pkts["pkt_len"][: 8] = (21, 400, 21, 400, 34, 33, 35, 400)
    offs = np.concatenate([[0], np.cumsum(pkts["pkt_len"][:-1].astype(np.int64) + 3)])
    pkts["pkt_off"], pkts["data_off"] = offs + 1, offs
    pkts["key"], pkts["hp_key"] = np.arange(m) % NKEYS, (np.arange(m) * 3) % NKEYS
    pkts["pn"] = np.arange(m)
    total = int(offs[-1]) + 512
    buf = rng.integers(0, 256, total, dtype=np.uint8)
    want_order = model.plan_order(pkts)
    assert len(set((model.lens(pkts) >> 4).tolist())) >= 10 and not np.array_equal(want_order, np.arange(m))
    rx = ptls_hip.QuicRx(engine, 0, m)
    try:
        load(rx, pkts)
        runs = {}
        for mode in (ptls_hip.QUIC_RX_PLAN_HOST, ptls_hip.QUIC_RX_PLAN_DEVICE, ptls_hip.QUIC_RX_PLAN_AUTO):
            rx.set_plan(mode)
            o = runs[mode] = Opened(rx, ks, hp, dev(buf), total, total)
            assert o.sel == list(range(m)) and o.res == [U64] * m and o.rep.lanes == 64
            if mode == ptls_hip.QUIC_RX_PLAN_HOST:
                assert o.rep.planned_on_device == 0 and o.order is None
            else:
                assert o.rep.planned_on_device == 1 and np.array_equal(o.order, want_order)
                assert o.same_outputs(runs[ptls_hip.QUIC_RX_PLAN_HOST])
    finally:
        torch.cuda.synchronize()
        rx.close()


@pytest.mark.parametrize("algo", ["aes128", "chacha"])
def test_fallback_on_one_key(engine, keysets, algo):
    """64 equal-length packets on one key, mode auto: AES is planned on the host with the host planner's lanes, ChaCha on the
    device; the outputs are the reference's.  The lanes are the model's, and the inner batch's of the existing path"""
    ks, hp = keysets(algo)
    sp = [s for s in specs("one") if len(s.payload) == 1200][:1] * 64
    assert len(sp) == 64
    packets = protected(algo, sp)
    buf, pkts, pkt_total, out_total = spec_input(algo, sp, packets)
    q = ptls_hip.QuicBatch(engine, pkts, open=True)
    host_lanes, host_chacha = q.records().lanes, q.records().chacha_lanes
    q.close()
    ghash, blocks, runs, _, n = model.stats(pkts)
    assert host_lanes == model.choose_lanes(ghash, runs, n, engine.cu_count) != 64
    assert host_chacha == model.choose_chacha_lanes(blocks, n, engine.cu_count)
    rx = ptls_hip.QuicRx(engine, 0, 64)
    try:
        load(rx, pkts)
        o = Opened(rx, ks, hp, dev(buf), pkt_total, out_total)
        res = check(o, algo, buf, pkts, range(64), out_total)
        assert res == [1200] * 64
        if algo == "chacha":
            assert (o.rep.planned_on_device, o.rep.lanes) == (1, host_chacha)
        else:
            assert (o.rep.planned_on_device, o.rep.lanes) == (0, host_lanes) and o.order is None
            rx.set_plan(ptls_hip.QUIC_RX_PLAN_DEVICE)  # forced: the wave-per-record kernel, the same bytes
            f = Opened(rx, ks, hp, dev(buf), pkt_total, out_total)
            assert (f.rep.planned_on_device, f.rep.lanes) == (1, 64) and f.same_outputs(o)
    finally:
        torch.cuda.synchronize()
        rx.close()


def test_model_lanes_are_the_host_planners(engine):
    """for generated packet lists, the lanes ptls_hip_quic_batch_new plans with are the model's from its sums"""
    rng = random.Random(8)
    for n, nkeys, run, lo, hi in ((300, 64, 1, 3, 400), (300, 4, 19, 3, 400), (400, 4, 20, 3, 400), (640, 10, 64, 4200, 9000),
                                  (1280, 10, 128, 4200, 9000), (900, 3, 300, 4200, 9000), (2000, 1, 2000, 3, 1400), (2000, 1, 2000, 40, 41)):
        pkts = np.zeros(n, dtype=ptls_hip.QUIC_PACKET_DTYPE)
        pkts["pn_offset"] = [rng.choice((1, 9, 47)) for _ in range(n)]
        pkts["pkt_len"] = [int(po) + 17 + rng.randrange(lo, hi) for po in pkts["pn_offset"]]
        pkts["key"] = [(i // run) % nkeys for i in range(n)]
        q = ptls_hip.QuicBatch(engine, pkts, open=True)
        try:
            ghash, blocks, runs, _, _ = model.stats(pkts)
            assert q.records().lanes == model.choose_lanes(ghash, runs, n, engine.cu_count), (n, nkeys, run)
            assert q.records().chacha_lanes == model.choose_chacha_lanes(blocks, n, engine.cu_count), (n, nkeys, run)
        finally:
            q.close()


@pytest.mark.parametrize("algo", ["aes128", "chacha"])
def test_unprotected_resubmission(engine, keysets, algo):
    """a packet sealed under key B fails under key A; its descriptor goes in again with PTLS_HIP_QUIC_UNPROTECTED and key B,
    through rx_set_packets, and opens: the header is read as it stands and no byte of the packet buffer changes"""
    ks, hp = keysets(algo)
    sp = specs("many")[::4]
    j, key_a = len(sp) // 2, 33
    assert sp[j].slot != key_a
    packets = protected(algo, sp)
    slots_a = [key_a if i == j else s.slot for i, s in enumerate(sp)]
    buf, pkts, pkt_total, out_total = spec_input(algo, sp, packets, 0, slots_a)
    rx = ptls_hip.QuicRx(engine, 0, len(sp))
    try:
        load(rx, pkts)
        d_buf = dev(buf)
        first = Opened(rx, ks, hp, d_buf, pkt_total, out_total)
        res = check(first, algo, buf, pkts, range(len(sp)), out_total)
        assert [i for i, r in enumerate(res) if r == U64] == [j]
        again = pkts[j: j + 1].copy()
        again["key"], again["flags"] = sp[j].slot, ptls_hip.QUIC_UNPROTECTED
        load(rx, again)
        second = Opened(rx, ks, hp, d_buf, pkt_total, out_total)
        assert check(second, algo, first.pkt, again, [0], out_total) == [len(sp[j].payload)]
        assert np.array_equal(second.pkt, first.pkt) and second.pns == [sp[j].pn]
    finally:
        torch.cuda.synchronize()
        rx.close()


def test_empty_cases_and_refusals_with_real_keysets(engine, keysets):
    ks, hp = keysets("aes128")
    ks256, hp256 = keysets("aes256")
    ksc, hpc = keysets("chacha")
    other = ptls_hip.Engine(0)
    foreign = ptls_hip.KeySet(other, 16, 4)
    pkts, info = boundary_descriptors(70000, 70000)
    buf = np.random.default_rng(1).integers(0, 256, 70256, dtype=np.uint8)
    rx = ptls_hip.QuicRx(engine, 0, len(pkts))
    L = ptls_hip.lib()
    try:
        d_buf = dev(buf)
        # nothing loaded: 0, nothing selected, whatever the buffers
        rep = ptls_hip.QuicRxReport(9, 9, 9)
        assert L.ptls_hip_quic_rx_open(rx.ptr, ks.ptr, hp.ptr, ALL, None, 0, None, 0, None, None, None, ctypes.addressof(rep), None) == 0
        assert (rep.n_selected, rep.planned_on_device, rep.lanes) == (0, 0, 0)
        # entries, none selectable: no connection anywhere, then a mask that matches no entry
        none = pkts.copy()
        none["key"] = ptls_hip.QUIC_NO_CONN
        for p, f, mask in ((none, None, ALL), (pkts, info, 1 << 20), (pkts, info, 0)):
            load(rx, p, f)
            o = Opened(rx, ks, hp, d_buf, 70000, 70000, mask=mask)
            assert o.m == 0 and o.sel == [] and (o.out == FILL).all() and np.array_equal(o.pkt, buf) and o.order is None
            assert o.rep.planned_on_device == 0
        # refusals: nothing launched, nothing written
        load(rx, pkts, info)
        d_out = torch.full((70000,), FILL, dtype=torch.uint8, device="cuda")
        d_sel = torch.zeros(len(pkts) + 8, dtype=torch.int32, device="cuda")
        d_res = torch.full((len(pkts) + 8,), SENTINEL, dtype=torch.int64, device="cuda")

        def call(a=ks, h=hp, b=d_buf.data_ptr(), bl=70000, o=d_out.data_ptr(), ol=70000, s=d_sel.data_ptr(), r=d_res.data_ptr(),
                 pn=d_res.data_ptr()):
            return L.ptls_hip_quic_rx_open(rx.ptr, a.ptr, h.ptr, ALL, b, bl, o, ol, s, r, pn, ctypes.addressof(rep), None)

        for kw, msg in ((dict(a=foreign), "same engine"), (dict(h=foreign), "same engine"), (dict(h=hp256), "algorithm and key size"),
                        (dict(a=ks256), "algorithm and key size"), (dict(a=ksc), "algorithm and key size"),
                        (dict(h=hpc), "algorithm and key size"), (dict(b=None), "null buffer"), (dict(o=None), "null buffer"),
                        (dict(s=None), "null buffer"), (dict(r=None), "null buffer"), (dict(pn=None), "null buffer"),
                        (dict(o=d_buf.data_ptr() + 69999, ol=16), "overlaps the packet buffer"),
                        (dict(o=d_buf.data_ptr(), ol=1), "overlaps the packet buffer")):
            assert call(**kw) == ptls_hip.EINVAL, kw
            assert "quic_rx_open:" in ptls_hip.last_error() and msg in ptls_hip.last_error(), (kw, ptls_hip.last_error())
        torch.cuda.synchronize()
        assert (d_out == FILL).all() and (d_res == SENTINEL).all() and (d_sel == 0).all() and np.array_equal(d_buf.cpu().numpy(), buf)
        assert call(o=d_buf.data_ptr() + 70000, ol=256) == 0  # adjacent, not overlapping
        torch.cuda.synchronize()
        with pytest.raises(ptls_hip.HipError, match="descriptors, the receive object holds"):
            rx.set_packets(d_buf, None, len(pkts) + 1)
        with pytest.raises(ptls_hip.HipError, match="a mode other than 0"):
            rx.set_plan(3)
    finally:
        torch.cuda.synchronize()
        rx.close()
        foreign.close()
        other.close()
