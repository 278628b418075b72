"""QUIC datagrams parsed on the GPU (include/ptls_hip.h 2h; hsig-picotls_amd/csrc/quic_parse_kernel.hip), bit-exact against the
plain-Python reference (tests/quic_parse_ref.py).  No tolerance anywhere: every comparison is whole arrays of packet
descriptors and info records against the reference's.  The host arrays start sentinel-filled with room for 8 more entries
than needed, and the tail must come back untouched.

Datagrams lie at odd offsets with 1- to 64-byte gaps, and the gap bytes are bait: behind a truncated datagram they are the
bytes the truncation cut off (the rest of a varint, a Length, a DCID that is in the map), so a kernel that reads past a
datagram's end produces a wrong entry instead of a fault, while the expected output stays the reference's TRUNCATED.

The scan's seams (test_counts_across_the_scan_seams): one scan workgroup spans QP_SCAN_SPAN = 2048 counts (256 threads x 8),
so n = 2049 is the first size with a second scan level, and the second level spans 2048 * 2048 = 4 194 304 datagrams, so
n = 4 194 305 is the first with a third."""
import ctypes
import random

import numpy as np
import pytest
import torch

import ptls_hip
import quic_keys_ref
import quic_parse_cases as gen
import quic_parse_ref as ref
import quic_ref
from test_gpu_quic import ALGO_OF, FILL, SENTINEL, U64, key_material, keysets  # noqa: F401 (keysets: a fixture)

pytestmark = pytest.mark.gpu
SENT = 0xC3
SPAN = 2048


def sentinel_arrays(cap):
    pkts = np.full(cap * 40, SENT, dtype=np.uint8).view(ptls_hip.QUIC_PACKET_DTYPE)
    info = np.full(cap * 32, SENT, dtype=np.uint8).view(ptls_hip.QUIC_PKTINFO_DTYPE)
    return pkts, info


def parse_raw(engine, dgrams, d_buf, buf_len, cap, cmap=None, scl=0, mx=16, fixed=1, expected=None, expected_count=0):
    """one call with sentinel-filled arrays of `cap` entries: (rc, n_pkts, pkts, info), the arrays whole"""
    dgrams = np.ascontiguousarray(dgrams, dtype=ptls_hip.QUIC_DATAGRAM_DTYPE)
    params = ptls_hip.QuicParseParams(scl, mx, fixed, 0, expected.data_ptr() if expected is not None else None, expected_count)
    pkts, info = sentinel_arrays(cap)
    n_pkts = ctypes.c_size_t(0xDEAD)
    rc = ptls_hip.lib().ptls_hip_quic_parse_datagrams(
        engine.ptr, ctypes.addressof(params), cmap.ptr if cmap is not None else None, dgrams.ctypes.data, len(dgrams),
        d_buf.data_ptr(), buf_len, pkts.ctypes.data, info.ctypes.data, cap, ctypes.byref(n_pkts),
        torch.cuda.current_stream().cuda_stream)
    return rc, n_pkts.value, pkts, info


def parse_checked(engine, dgrams, d_buf, buf_len, want, **kw):
    """the sizing call (cap 0), then the call with 8 entries to spare: exactly the reference's entries, the tail untouched"""
    want_pkts, want_info = want
    n = len(want_pkts)
    if n != 0:
        rc, need, _, _ = parse_raw(engine, dgrams, d_buf, buf_len, 0, **kw)
        assert rc == ptls_hip.EINVAL and need == n, (rc, need, n, ptls_hip.last_error())
    rc, got, pkts, info = parse_raw(engine, dgrams, d_buf, buf_len, n + 8, **kw)
    assert rc == 0, ptls_hip.last_error()
    assert got == n
    assert np.array_equal(pkts[:n], want_pkts), first_difference(pkts[:n], want_pkts)
    assert np.array_equal(info[:n], want_info), first_difference(info[:n], want_info)
    assert (pkts[n:].view(np.uint8) == SENT).all() and (info[n:].view(np.uint8) == SENT).all()
    return pkts[:n], info[:n]


def first_difference(got, want):
    for k in range(min(len(got), len(want))):
        if got[k] != want[k]:
            return "entry %d: got %s, want %s" % (k, got[k], want[k])
    return "lengths %d / %d" % (len(got), len(want))


def lay_out(cases, seed):
    """datagrams at odd offsets with gaps of 1 .. 64 bytes that start with each datagram's bait: (buffer, datagram array)"""
    rng = random.Random(seed)
    buf = bytearray(rng.randbytes(3))
    dg = np.zeros(len(cases), dtype=ptls_hip.QUIC_DATAGRAM_DTYPE)
    for i, (d, bait) in enumerate(cases):
        if len(buf) % 2 == 0:
            buf += rng.randbytes(1)
        dg["off"][i], dg["len"][i] = len(buf), len(d)
        gap = 1 + (i * 7) % 64
        # what an over-read would find: the cut-off bytes, then the start of a packet for a connection in the map
        lure = bait + gen.long_packet(rng, ref.V1, ref.HANDSHAKE, gen.CID_POOL[2], gen.CID_POOL[4])[0]
        buf += d + lure[:gap]
    buf += rng.randbytes(64)
    return np.frombuffer(bytes(buf), np.uint8).copy(), dg


def pool_map(engine):
    """the generator's connection IDs of up to 20 bytes, on the device and in the model"""
    model = ref.CidMap(32)
    for k, cid in enumerate(gen.CID_POOL):
        model.set(cid, 1000 + k)
    m = ptls_hip.QuicCidMap(engine, 32)
    m.set(list(model.d), list(model.d.values()))
    assert len(m) == len(model)
    return m, model


def reference(buf, dg, **kw):
    return ref.to_arrays(ref.parse_datagrams(bytes(buf), [(int(o), int(n)) for o, n in zip(dg["off"], dg["len"])], **kw))


@pytest.fixture(scope="module")
def parity_input():
    cases = list(gen.cases(seed=4242, random_fill=400))
    picked = cases[::11] + [c for c in cases if c[1]][5::9][:60]  # a spread of every family, and more of the truncated ones
    assert 280 <= len(picked) <= 420 and sum(1 for _, bait in picked if bait) >= 100
    return lay_out(picked, 1)


@pytest.mark.parametrize("scl,mx,fixed", [(8, 16, 1), (0, 3, 0), (20, 1, 1)])
def test_parity_with_bait_behind_every_datagram(engine, parity_input, scl, mx, fixed):
    buf, dg = parity_input
    d_buf = torch.from_numpy(buf).cuda()
    m, model = pool_map(engine)
    try:
        want = reference(buf, dg, short_cid_len=scl, max_per_dgram=mx, require_fixed_bit=fixed, cidmap=model)
        statuses = set(want[1]["status"].tolist())
        assert statuses >= {ref.OK, ref.TRUNCATED} and (want[1]["conn"] != ref.NO_CONN).any()
        a = parse_checked(engine, dg, d_buf, len(buf), want, cmap=m, scl=scl, mx=mx, fixed=fixed)
        b = parse_checked(engine, dg, d_buf, len(buf), want, cmap=m, scl=scl, mx=mx, fixed=fixed)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()  # the same input, the same bytes
        assert np.array_equal(d_buf.cpu().numpy(), buf)  # the parse only reads
        # the binding's own call
        pkts, info = ptls_hip.quic_parse_datagrams(engine, dg, d_buf, len(buf), cidmap=m, short_cid_len=scl, max_per_dgram=mx,
                                                   require_fixed_bit=fixed)
        assert np.array_equal(pkts, want[0]) and np.array_equal(info, want[1])
    finally:
        m.close()


def counting_pool(mx):
    """mx + 1 kinds of datagram: kind c holds c packets, kind mx one more than fits (MORE); (buffer, [(off, len)] per kind)"""
    rng = random.Random(mx)
    buf, kinds = bytearray(b"\x99"), [(0, 0)]
    for c in range(1, mx + 1):
        d = b"".join(gen.long_packet(rng, ref.V1, ref.HANDSHAKE, gen.CID_POOL[2], b"", body_len=20 + c)[0]
                     for _ in range(c + (1 if c == mx else 0)))
        kinds.append((len(buf), len(d)))
        buf += d + b"\x99" * 3
    return np.frombuffer(bytes(buf), np.uint8).copy(), kinds


@pytest.mark.parametrize("n,mx", [(0, 3), (1, 3), (63, 3), (64, 3), (65, 3), (255, 3), (256, 3), (257, 3), (SPAN + 1, 16),
                                  (SPAN * SPAN + 1, 1)])
def test_counts_across_the_scan_seams(engine, n, mx):
    """n datagrams whose entry counts cycle through 0 .. mx (0: a zero-length datagram; mx: with MORE), n on both sides of a
    wave, of a workgroup, of one scan span (2048) and of the second scan level's span (2048 * 2048): n_pkts, the order and the
    dgram indices"""
    buf, kinds = counting_pool(mx)
    d_buf = torch.from_numpy(buf).cuda()
    per_kind = [reference(buf, np.array([(o, ln, 0)], dtype=ptls_hip.QUIC_DATAGRAM_DTYPE), short_cid_len=8, max_per_dgram=mx)
                for o, ln in kinds]
    assert [len(p) for p, _ in per_kind] == list(range(mx + 1))
    assert per_kind[mx][1]["flags"][-1] == ref.MORE and (mx == 1 or per_kind[1][1]["flags"][-1] == 0)
    kind = np.arange(n) % (mx + 1)
    dg = np.zeros(n, dtype=ptls_hip.QUIC_DATAGRAM_DTYPE)
    dg["off"], dg["len"] = np.array([o for o, _ in kinds])[kind], np.array([ln for _, ln in kinds])[kind]
    # the expected arrays: whole cycles of the kinds' entries, then the rest, with the datagram index filled in
    cyc_p, cyc_i = np.concatenate([p for p, _ in per_kind]), np.concatenate([f for _, f in per_kind])
    full, part = divmod(n, mx + 1)
    tail = sum(range(part))
    want_p = np.concatenate([np.tile(cyc_p, full), cyc_p[:tail]])
    want_i = np.concatenate([np.tile(cyc_i, full), cyc_i[:tail]])
    want_i["dgram"] = np.repeat(np.arange(n, dtype=np.uint32), kind)
    assert len(want_p) == int(kind.sum())
    parse_checked(engine, dg, d_buf, len(buf), (want_p, want_i), scl=8, mx=mx)


def test_cap_too_small(engine):
    buf, kinds = counting_pool(3)
    d_buf = torch.from_numpy(buf).cuda()
    dg = np.array([(o, ln, 0) for o, ln in kinds * 5], dtype=ptls_hip.QUIC_DATAGRAM_DTYPE)
    need = 5 * 6
    for cap in (need - 1, 1, 0):
        rc, got, pkts, info = parse_raw(engine, dg, d_buf, len(buf), cap, mx=3)
        assert rc == ptls_hip.EINVAL and got == need
        assert "%d entries do not fit the arrays of %d" % (need, cap) in ptls_hip.last_error()
        assert (pkts.view(np.uint8) == SENT).all() and (info.view(np.uint8) == SENT).all()
    rc, got, _, _ = parse_raw(engine, dg, d_buf, len(buf), need, mx=3)
    assert rc == 0 and got == need


def chain(size, home, count, length):
    out, k = [], 0
    while len(out) < count:
        cid = k.to_bytes(length, "big")
        if ref.cid_hash(cid) & (size - 1) == home:
            out.append(cid)
        k += 1
    return out


def cid_datagrams(cids, seed):
    """per CID one datagram: a Handshake packet with it as the DCID coalesced with, for 8-byte CIDs, a short-header packet"""
    rng = random.Random(seed)
    out = []
    for cid in cids:
        d = gen.long_packet(rng, rng.choice((ref.V1, ref.V2)), ref.HANDSHAKE, cid, b"\x01\x02")[0]
        if len(cid) == 8:
            d += gen.short_packet(rng, cid)
        out.append((d, b""))
    return out


def test_cid_map_on_the_device(engine):
    """capacity 8 (16 slots) with CIDs that collide in the table's last slot and wrap around its end; set, replace and remove
    between parse calls; lookups through long and short headers; a null map"""
    colliding = chain(16, 15, 4, 8) + chain(16, 0, 2, 8)
    others = [b"", bytes(range(20))]
    absent = chain(16, 15, 6, 8)[4:] + [bytes(20), b"\x05"]
    buf, dg = lay_out(cid_datagrams(colliding + others + absent, 3), 4)
    d_buf = torch.from_numpy(buf).cuda()
    m, model = ptls_hip.QuicCidMap(engine, 8), ref.CidMap(8)

    def check():
        assert len(m) == len(model)
        want = reference(buf, dg, short_cid_len=8, cidmap=model)
        _, info = parse_checked(engine, dg, d_buf, len(buf), want, cmap=m, scl=8)
        return info

    try:
        assert (check()["conn"] == ref.NO_CONN).all()  # the empty map
        for k, cid in enumerate(colliding + others):
            model.set(cid, 10 + k)
        m.set(colliding + others, [10 + k for k in range(8)])
        info = check()
        assert sorted(set(info["conn"].tolist())) == list(range(10, 18)) + [ref.NO_CONN]
        with pytest.raises(ptls_hip.HipError, match="exceed the capacity of 8"):
            m.set([absent[0]], [99])  # full
        model.set(colliding[1], 77)  # replace
        m.set([colliding[1]], [77])
        check()
        for victim in (colliding[0], colliding[3], colliding[1], others[0]):  # the chain's head, its tail, its middle
            model.remove(victim)
            m.remove([victim, absent[1]])  # (an absent CID with it: not an error)
            check()
        model.set(absent[0], 5)
        model.set(colliding[0], 6)
        m.set([absent[0], colliding[0]], [5, 6])
        check()
        want = reference(buf, dg, short_cid_len=8, cidmap=None)
        assert (want[1]["conn"] == ref.NO_CONN).all() and (want[0]["key"] == ref.NO_CONN).all()
        parse_checked(engine, dg, d_buf, len(buf), want, cmap=None, scl=8)
    finally:
        m.close()


def test_cid_map_of_64k_entries(engine):
    rng = random.Random(64)
    n = 1 << 16
    cids = list({rng.randbytes(8) for _ in range(n)})
    model = ref.CidMap(n)
    for k, cid in enumerate(cids):
        model.set(cid, k * 3)
    m = ptls_hip.QuicCidMap(engine, n)
    try:
        m.set(cids, [k * 3 for k in range(len(cids))])
        m.remove(cids[::5])
        for cid in cids[::5]:
            model.remove(cid)
        assert len(m) == len(model)
        picked = [rng.choice(cids) if i % 9 else rng.randbytes(8) for i in range(4096)]
        buf, dg = lay_out([(gen.short_packet(rng, cid, 21 + i % 40), b"") for i, cid in enumerate(picked)], 6)
        d_buf = torch.from_numpy(buf).cuda()
        want = reference(buf, dg, short_cid_len=8, cidmap=model)
        assert 2500 < int((want[1]["conn"] != ref.NO_CONN).sum()) < 3500  # 8 of 9 picked from the set, a fifth of it removed
        parse_checked(engine, dg, d_buf, len(buf), want, cmap=m, scl=8)
    finally:
        m.close()


def test_expected_packet_numbers(engine):
    """pn = d_expected_pn[3 conn + space] for the three spaces of two connections; an index at expected_count and beyond
    gives 0; so does a null table, a packet without a connection, and an entry that is not openable"""
    rng = random.Random(12)
    a, b, c = bytes(range(8)), bytes(range(30, 38)), bytes(range(60, 68))
    cases = []
    for cid in (a, b, c):
        d = b"".join(gen.long_packet(rng, v, t, cid, b"")[0] for v, t in ((ref.V1, ref.INITIAL), (ref.V2, ref.ZERO_RTT),
                                                                         (ref.V1, ref.HANDSHAKE), (ref.V2, ref.RETRY)))
        cases += [(d, b""), (gen.short_packet(rng, cid), b"")]
    buf, dg = lay_out(cases, 8)
    d_buf = torch.from_numpy(buf).cuda()
    table = [(1 << 61) + 5, 7, (1 << 40) + 1, 11, 0xFFFFFFFFFFFF, 13]
    d_table = torch.tensor(np.array(table, dtype=np.uint64).view(np.int64), device="cuda")
    m, model = ptls_hip.QuicCidMap(engine, 4), ref.CidMap(4)
    try:
        for cid, conn in ((a, 0), (b, 1)):
            model.set(cid, conn)
        m.set([a, b], [0, 1])
        for count in (6, 5, 4, 3, 1, 0):
            want = reference(buf, dg, short_cid_len=8, cidmap=model, expected_pn=table, expected_count=count)
            parse_checked(engine, dg, d_buf, len(buf), want, cmap=m, scl=8, expected=d_table, expected_count=count)
            if count == 6:
                assert sorted(set(want[0]["pn"].tolist())) == sorted(set(table + [0]))
        want = reference(buf, dg, short_cid_len=8, cidmap=model)
        assert (want[0]["pn"] == 0).all()
        parse_checked(engine, dg, d_buf, len(buf), want, cmap=m, scl=8, expected=None, expected_count=6)
    finally:
        m.close()


NCONN = 12
E2E_CIDS = [bytes([0xB0 + c]) + bytes(range(c, c + 7)) for c in range(NCONN)]


def e2e_packet(rng, algo, conn, kind, expected_pn, keys=None):
    """one protected packet of connection `conn`: (bytes, the unprotected header, packet number, payload)"""
    pn_len = rng.randrange(1, 5)
    pn = expected_pn + rng.randrange(0, 100)
    payload = rng.randbytes(rng.choice((3, 16, 17, 64, 255, 1200)))
    trunc = (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big")
    cid = E2E_CIDS[conn] if conn is not None else keys[3]
    if kind == ref.ONE_RTT:
        header = bytes([0x40 | rng.randrange(8) << 2 | (pn_len - 1)]) + cid + trunc
    else:
        version = rng.choice((ref.V1, ref.V2)) if keys is None else ref.V1
        first = 0xC0 | gen.TYPE_BITS[version][kind] << 4 | (pn_len - 1)
        header = bytes([first]) + version.to_bytes(4, "big") + bytes([len(cid)]) + cid + b"\x04" + rng.randbytes(4)
        if kind == ref.INITIAL:
            token = rng.randbytes(rng.choice((0, 7, 70)))
            header += gen.varint(len(token)) + token
        header += gen.varint(pn_len + len(payload) + 16, rng.choice((2, 4))) + trunc
    if keys is None:
        ks, ivs, hps = key_material(algo)
        key, iv, hp = ks[conn], ivs[conn], hps[conn]
    else:
        key, iv, hp = keys[:3]
    return quic_ref.protect(algo, key, iv, hp, header, pn, payload), header, pn, payload


def open_parsed(engine, ks, hp, pkts, d_buf, total):
    """the parsed descriptors straight into an open batch: (results, packet numbers, the packet buffer after, the output)"""
    d_out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    d_res = torch.full((len(pkts),), SENTINEL, dtype=torch.int64, device="cuda")
    d_pn = torch.full((len(pkts),), SENTINEL, dtype=torch.int64, device="cuda")
    q = ptls_hip.QuicBatch(engine, pkts, open=True)
    try:
        q.open(ks, hp, d_buf, d_out, d_res, d_pn)
        torch.cuda.synchronize()
    finally:
        q.close()
    return ([int(x) & U64 for x in d_res.cpu().tolist()], [int(x) & U64 for x in d_pn.cpu().tolist()], d_buf.cpu().numpy(),
            d_out.cpu().numpy())


def check_opened(buf, pkts, sent, res, pns, pkt_after, out):
    """sent[k] = (bytes, header, pn, payload) of parsed packet k"""
    assert res == [len(s[3]) for s in sent] and pns == [s[2] for s in sent]
    want_pkt, want_out = buf.copy(), np.full(len(buf), FILL, np.uint8)
    for p, (_, header, _, payload) in zip(pkts, sent):
        o = int(p["pkt_off"])
        want_pkt[o: o + len(header)] = np.frombuffer(header, np.uint8)
        want_out[int(p["data_off"]): int(p["data_off"]) + len(payload)] = np.frombuffer(payload, np.uint8)
    assert np.array_equal(pkt_after, want_pkt)
    assert np.array_equal(out, want_out)


@pytest.mark.parametrize("algo", ["aes128", "aes256", "chacha"])
def test_end_to_end_parse_then_open(engine, keysets, algo):
    """packets protected by the reference, packed into datagrams (some coalesced, some for connections the map does not know,
    a Retry among them), parsed on the device; the openable entries with a connection go straight into QuicBatch(open)"""
    rng = random.Random(ALGO_OF[algo][1] + len(algo))
    ks, hp = keysets(algo)
    base = [[(1 << 33) + 1000 * c, 50 + c, (1 << 20) * c + 7] for c in range(NCONN)]  # expected pn per connection and space
    datagrams, sent_by_off = [], {}
    for i in range(40):
        conn = i % NCONN
        kinds = [(ref.HANDSHAKE, ref.ONE_RTT), (ref.ONE_RTT,), (ref.ZERO_RTT, ref.HANDSHAKE, ref.ONE_RTT), (ref.INITIAL, ref.HANDSHAKE)][i % 4]
        made = [e2e_packet(rng, algo, conn, k, base[conn][ref.pn_space(k)]) for k in kinds]
        datagrams.append(made)
    layout_cases = []
    for i, made in enumerate(datagrams):
        d = b"".join(m[0] for m in made)
        if i % 10 == 3:  # a connection the map does not know, and a Retry: parsed, not opened
            d = gen.long_packet(rng, ref.V1, ref.HANDSHAKE, b"\xEE" * 8, b"")[0] + d
        if i % 20 == 7:  # (behind a long header: a short one would take the rest of the datagram)
            d = d + gen.long_packet(rng, ref.V1, ref.RETRY, E2E_CIDS[0], b"")[0]
        layout_cases.append((d, b""))
    buf, dg = lay_out(layout_cases, 21)
    for i, made in enumerate(datagrams):
        pos = int(dg["off"][i]) + (len(layout_cases[i][0]) - sum(len(m[0]) for m in made) if i % 10 == 3 else 0)
        for m in made:
            sent_by_off[pos] = m
            pos += len(m[0])
    d_buf = torch.from_numpy(buf).cuda()
    model = ref.CidMap(NCONN)
    for c, cid in enumerate(E2E_CIDS):
        model.set(cid, c)
    m = ptls_hip.QuicCidMap(engine, NCONN)
    flat = [v for row in base for v in row]
    d_expected = torch.tensor(np.array(flat, dtype=np.uint64).view(np.int64), device="cuda")
    try:
        m.set(E2E_CIDS, list(range(NCONN)))
        want = reference(buf, dg, short_cid_len=8, cidmap=model, expected_pn=flat)
        pkts, info = parse_checked(engine, dg, d_buf, len(buf), want, cmap=m, scl=8, expected=d_expected, expected_count=len(flat))
    finally:
        m.close()
    openable = (pkts["pn_offset"] != 0) & (info["conn"] != ref.NO_CONN)
    assert int(openable.sum()) == len(sent_by_off) and int((~openable).sum()) == 6
    mine = np.ascontiguousarray(pkts[openable])
    sent = [sent_by_off[int(o)] for o in mine["pkt_off"]]
    check_opened(buf, mine, sent, *open_parsed(engine, ks, hp, mine, d_buf, len(buf)))
    # the rest is refused by name, not opened under slot 0
    with pytest.raises(ptls_hip.HipError):
        open_parsed(engine, ks, hp, np.ascontiguousarray(pkts[(pkts["pn_offset"] != 0) & ~openable]), d_buf, len(buf))
    assert "names key slot 4294967295" in ptls_hip.last_error()


def test_initial_packets_of_unknown_connections(engine):
    """client Initials under DCIDs the map does not hold: the DCID is read back through dcid_off / dcid_len, the Initial keys
    are derived on the device from it (2f), and the packets open"""
    rng = random.Random(2)
    dcids = [rng.randbytes(n) for n in (8, 8, 20, 1, 13)]
    sent_all, cases = [], []
    for dcid in dcids:
        client, _ = quic_keys_ref.initial_secrets(quic_keys_ref.V1_SALT, dcid)
        key, iv, hp = quic_keys_ref.keys(client, 16)
        made = [e2e_packet(rng, "aes128", None, ref.INITIAL, 0, keys=(key, iv, hp, dcid)) for _ in range(2)]
        sent_all += made
        cases.append((b"".join(s[0] for s in made), b""))
    buf, dg = lay_out(cases, 33)
    d_buf = torch.from_numpy(buf).cuda()
    m = ptls_hip.QuicCidMap(engine, 4)
    try:
        m.set([b"\x01" * 8], [3])
        pkts, info = ptls_hip.quic_parse_datagrams(engine, dg, d_buf, len(buf), cidmap=m, short_cid_len=8)
    finally:
        m.close()
    assert len(pkts) == 10 and (info["type"] == ref.INITIAL).all() and (info["conn"] == ref.NO_CONN).all()
    assert (info["status"] == ref.OK).all() and (pkts["pn_offset"] != 0).all()
    seen = []
    for p, f in zip(pkts, info):
        o = int(p["pkt_off"]) + int(f["dcid_off"])
        dcid = buf[o: o + int(f["dcid_len"])].tobytes()
        if dcid not in seen:
            seen.append(dcid)
        p["key"] = p["hp_key"] = 2 * seen.index(dcid)  # the client's keys (slot 2 i; the server's are 2 i + 1)
    assert seen == dcids
    ks, hp = ptls_hip.KeySet(engine, 16, 2 * len(seen)), ptls_hip.KeySet(engine, 16, 2 * len(seen))
    try:
        ks.set_quic_initial(hp, 0, seen, quic_keys_ref.V1_SALT)
        check_opened(buf, pkts, sent_all, *open_parsed(engine, ks, hp, pkts, d_buf, len(buf)))
    finally:
        torch.cuda.synchronize()
        ks.close()
        hp.close()


def test_refusals_that_need_a_device(engine):
    """a datagram past buf_len, a len of 65536, a map of another engine: nothing launched, nothing written, the message names
    the datagram"""
    buf, kinds = counting_pool(3)
    d_buf = torch.from_numpy(buf).cuda()
    dg = np.array([(o, ln, 0) for o, ln in kinds], dtype=ptls_hip.QUIC_DATAGRAM_DTYPE)
    last = int(dg["off"][3] + dg["len"][3])
    m = ptls_hip.QuicCidMap(engine, 4)
    other = ptls_hip.Engine(0)
    foreign = ptls_hip.QuicCidMap(other, 4)
    try:
        m.set([b"abc"], [1])
        foreign.set([b"abc"], [1])
        for kw, dgrams, buf_len, msg in (
                (dict(cmap=m), dg, last - 1, "datagram 3: off %d + len %d is past the buffer of %d bytes" % (dg["off"][3], dg["len"][3], last - 1)),
                (dict(cmap=m), np.array([(0, 1, 0), (0, 65536, 0)], dtype=dg.dtype), 1 << 20, "datagram 1: len 65536 is above 65535"),
                (dict(cmap=foreign), dg, len(buf), "belongs to another engine")):
            rc, got, pkts, info = parse_raw(engine, dgrams, d_buf, buf_len, 16, mx=3, **kw)
            assert rc == ptls_hip.EINVAL and got == 0xDEAD and msg in ptls_hip.last_error(), ptls_hip.last_error()
            assert (pkts.view(np.uint8) == SENT).all() and (info.view(np.uint8) == SENT).all()
        rc, got, _, _ = parse_raw(engine, dg, d_buf, last, 16, mx=3, cmap=m)  # exactly to the buffer's end: fine
        assert rc == 0 and got == 6
        rc, got, _, _ = parse_raw(other, dg, d_buf, last, 16, mx=3, cmap=foreign)
        assert rc == 0 and got == 6
    finally:
        m.close()
        foreign.close()
        other.close()
