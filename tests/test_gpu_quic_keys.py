"""QUIC packet-protection keys derived on the GPU (include/ptls_hip.h 2f; hsig-picotls_amd/csrc/quic_keys.hip), checked against
Python's HKDF with the reference's Expand-Label (tests/quic_keys_ref.py) and against RFC 9001 Appendix A.  Keys cannot be read
back from a keyset, so a keyset is judged by what it does, slot by slot (`behaviour`): its static IVs, a 1..40-byte record
sealed under every slot, and the header-protection mask of a fixed sample under every slot.  All three must equal those of a
keyset pair loaded with ptls_hip_keyset_set from the expected raw keys, and the masks must equal quic_ref.hp_mask.  No
tolerance anywhere: every comparison is of whole byte strings."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import ptls_hip
import quic_keys_ref as kr
import quic_ref

pytestmark = pytest.mark.gpu
U64 = (1 << 64) - 1
SENTINEL = 0x5a5a5a5a5a5a5a5a
FILL = 0xA5
# name -> (algorithm, key size, hash size)
ALGOS = {"aes128": (ptls_hip.ALGO_AESGCM, 16, 32), "aes256": (ptls_hip.ALGO_AESGCM, 32, 48),
         "chacha": (ptls_hip.ALGO_CHACHA20POLY1305, 32, 32)}
A2_SAMPLE = bytes.fromhex("d1b1c98dd7689fb8ec11d242b123dc9b")


def stream(tag, n):
    out, i = bytearray(), 0
    while len(out) < n:
        out += hashlib.sha256(b"%s/%d" % (tag.encode(), i)).digest()
        i += 1
    return bytes(out[:n])


def dev(buf):
    return torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).cuda()


def new_pair(engine, algo, nslots):
    kind, ksz, _ = ALGOS[algo]
    return ptls_hip.KeySet(engine, ksz, nslots, algo=kind), ptls_hip.KeySet(engine, ksz, nslots, algo=kind)


def old_material(algo, nslots, tag="old"):
    """raw (key, iv, hp) per slot of a keyset pair before the call under test"""
    ksz = ALGOS[algo][1]
    return [(stream("%s-%s-key-%d" % (tag, algo, i), ksz), stream("%s-%s-iv-%d" % (tag, algo, i), 12),
             stream("%s-%s-hp-%d" % (tag, algo, i), ksz)) for i in range(nslots)]


def load(pair, first, material):
    """ptls_hip_keyset_set of both keysets from raw (key, iv, hp) triples"""
    ks, hp = pair
    ks.set(first, b"".join(m[0] for m in material), b"".join(m[1] for m in material))
    hp.set(first, b"".join(m[2] for m in material), None)


def masks(engine, algo, hp, slots, sample=None):
    """the 16-byte header-protection block of a fixed sample per slot (ptls_hip_aesecb_batch / _chacha20_mask_batch)"""
    n = len(slots)
    samples = [sample or stream("sample-%d" % s, 16) for s in slots]
    supp = np.zeros(n, dtype=ptls_hip.SUPP_DTYPE)
    supp["sample_off"] = supp["mask_off"] = np.arange(n) * 16
    supp["hp_key"], supp["flags"] = slots, ptls_hip.SUPP_ENABLE
    d_supp = torch.from_numpy(supp.view(np.uint8).copy()).cuda()
    d_mask = torch.full((n * 16,), FILL, dtype=torch.uint8, device="cuda")
    (engine.chacha20_mask if algo == "chacha" else engine.aesecb)(hp, d_supp, dev(b"".join(samples)), d_mask)
    torch.cuda.synchronize()
    out = d_mask.cpu().numpy().tobytes()
    return [out[16 * j: 16 * j + 16] for j in range(n)], samples


def behaviour(engine, algo, pair):
    """(static IVs, sealed records, masks) of every slot of the pair"""
    ks, hp = pair
    n = ks.nslots
    slots = list(range(n))
    lens = [1 + (s * 7) % 40 for s in slots]
    assert set(lens) == set(range(1, 41)) or n < 40
    recs, in_bytes, out_bytes, aad_bytes = ptls_hip.layout_records(lens, [5] * n, slots, [s + 1 for s in slots])
    d_in, d_aad = dev(stream("records", in_bytes)), dev(stream("aad", aad_bytes))
    d_out = torch.zeros(out_bytes, dtype=torch.uint8, device="cuda")
    b = ptls_hip.Batch(engine, recs)
    (b.chacha_seal if algo == "chacha" else b.seal)(ks, d_in, d_aad, d_out)
    torch.cuda.synchronize()
    b.close()
    sealed = d_out.cpu().numpy().tobytes()
    return [ks.get_iv(s) for s in slots], sealed, masks(engine, algo, hp, slots)[0]


def check_pair(engine, algo, pair, material, what):
    """the pair behaves as the raw (key, iv, hp) triples in `material`, one per slot"""
    n = pair[0].nslots
    assert len(material) == n
    ref = new_pair(engine, algo, n)
    load(ref, 0, material)
    ivs, sealed, mk = behaviour(engine, algo, pair)
    want_ivs, want_sealed, want_mk = behaviour(engine, algo, ref)
    for k in ref:
        k.close()
    assert ivs == [m[1] for m in material], (what, "get_iv")
    assert [pair[1].get_iv(s) for s in range(n)] == [bytes(12)] * n, (what, "hp get_iv")
    assert want_ivs == ivs
    assert sealed == want_sealed, (what, "sealed records")
    assert mk == want_mk, (what, "masks against the keyset loaded from raw keys")
    assert mk == [quic_ref.hp_mask(algo, m[2], stream("sample-%d" % s, 16)) for s, m in enumerate(material)], (what, "hp_mask")


def close(*pairs):
    torch.cuda.synchronize()
    for pair in pairs:
        for k in pair:
            k.close()


@pytest.mark.parametrize("labels", [1, 2])
@pytest.mark.parametrize("algo", ["aes128", "aes256", "chacha"])
def test_set_quic_secrets(engine, algo, labels):
    """first = 3, count = 130 in keysets of 140 slots holding other keys, then counts 1, 63, 64, 65 around the workgroup
    width with fresh secrets each: after every call all 140 slots of both keysets behave as expected -- the named range under
    the derived keys, every slot outside it (0..2, 133..139 for the first call) under what it held before"""
    _, ksz, hs = ALGOS[algo]
    pair = new_pair(engine, algo, 140)
    material = old_material(algo, 140)
    load(pair, 0, material)
    for count in (130, 1, 63, 64, 65):
        secrets = [stream("secret-%s-%d-%d-%d" % (algo, labels, count, i), hs) for i in range(count)]
        pair[0].set_quic_secrets(pair[1], 3, b"".join(secrets), hs, labels)
        material[3: 3 + count] = [kr.keys(s, ksz, labels == 2) for s in secrets]
        check_pair(engine, algo, pair, material, (algo, labels, count))
    close(pair)


A1_DCID = bytes.fromhex("8394c8f03e515708")
A1_CLIENT = tuple(bytes.fromhex(x) for x in ("1f369613dd76d5467730efcbe3b1a22d", "fa044b2f42a3fd3b46fb255c",
                                             "9f50449e04a0e810283a1e9933adedd2"))
A1_SERVER = tuple(bytes.fromhex(x) for x in ("cf3a5331653c364c88f0f379b6067e37", "0ac1493ca1905853b0bba03e",
                                             "c206b8d9b9f0f37644430b490eeaa314"))


def test_rfc9001_a1_initial_keys(engine):
    """RFC 9001 A.1: DCID 8394c8f03e515708 under the v1 salt gives the RFC's client and server key, IV and hp key, and the
    client slot's mask of A.2's sample is A.2's (437b9aec36, as in tests/test_quic_ref.py)"""
    pair = new_pair(engine, "aes128", 4)
    material = old_material("aes128", 4)
    load(pair, 0, material)
    pair[0].set_quic_initial(pair[1], 1, [A1_DCID], ptls_hip.QUIC_V1_SALT)
    assert pair[0].get_iv(1) == A1_CLIENT[1] and pair[0].get_iv(2) == A1_SERVER[1]
    material[1:3] = [A1_CLIENT, A1_SERVER]
    check_pair(engine, "aes128", pair, material, "A.1")
    mk, _ = masks(engine, "aes128", pair[1], [1], A2_SAMPLE)
    assert mk[0][:5] == bytes.fromhex("437b9aec36")
    assert mk[0] == quic_ref.hp_mask("aes128", A1_CLIENT[2], A2_SAMPLE)
    close(pair)


# ---- packets through the QUIC batches of 2e ----

def place(sizes):
    """odd offsets of consecutive pieces with gaps of 1 .. 64 bytes"""
    offs, pos = [], 0
    for i, s in enumerate(sizes):
        pos += 1 + (i * 7) % 64
        if pos % 2 == 0:
            pos += 1
        offs.append(pos)
        pos += s
    return offs, pos + 64


def image(total, offs, pieces):
    img = np.full(total, FILL, np.uint8)
    for o, p in zip(offs, pieces):
        img[o: o + len(p)] = np.frombuffer(p, np.uint8)
    return img


class Pkt:
    """one packet: header (first byte, pn_offset - 1 further bytes, the truncated packet number), packet number, payload"""

    def __init__(self, i, long_header):
        self.pn_len = 1 + i % 4
        self.pn = (1 << 32) * (i % 3) + 1000 + 7 * i
        self.expected = self.pn - (i % 5)  # what the receiver expects: within half a window of pn for every pn_len
        self.pn_offset = 18 if long_header else 9
        first = (0xc0 if long_header else 0x40) | (self.pn_len - 1)
        self.header = (bytes([first]) + stream("hdr-%d" % i, self.pn_offset - 1) +
                       (self.pn & ((1 << (8 * self.pn_len)) - 1)).to_bytes(self.pn_len, "big"))
        self.payload = stream("payload-%d" % i, 3 + (i * 11) % 48)
        self.pkt_len = len(self.header) + len(self.payload) + 16


def descriptors(pkts, pkt_offs, data_offs, slots, is_open):
    d = np.zeros(len(pkts), dtype=ptls_hip.QUIC_PACKET_DTYPE)
    d["pkt_off"], d["data_off"] = pkt_offs, data_offs
    d["pn"] = [p.expected if is_open else p.pn for p in pkts]
    d["pkt_len"] = [p.pkt_len for p in pkts]
    d["key"] = d["hp_key"] = slots
    d["pn_offset"] = [p.pn_offset for p in pkts]
    d["pn_len"] = [0 if is_open else p.pn_len for p in pkts]
    return d


def quic_open(engine, pair, pkts, wire, slots):
    """opens the protected packets `wire` under the pair's slots: (result, pn_out, plaintext per packet)"""
    pkt_offs, pkt_total = place([p.pkt_len for p in pkts])
    out_offs, out_total = place([len(p.payload) + 4 for p in pkts])
    d_pkt = torch.from_numpy(image(pkt_total, pkt_offs, wire)).cuda()
    d_out = torch.full((out_total,), FILL, dtype=torch.uint8, device="cuda")
    d_res = torch.full((len(pkts),), SENTINEL, dtype=torch.int64, device="cuda")
    d_pn = torch.full((len(pkts),), SENTINEL, dtype=torch.int64, device="cuda")
    q = ptls_hip.QuicBatch(engine, descriptors(pkts, pkt_offs, out_offs, slots, True), open=True)
    q.open(pair[0], pair[1], d_pkt, d_out, d_res, d_pn)
    torch.cuda.synchronize()
    q.close()
    out = d_out.cpu().numpy().tobytes()
    return ([int(x) & U64 for x in d_res.cpu().numpy().tolist()], [int(x) & U64 for x in d_pn.cpu().numpy().tolist()],
            [out[o: o + len(p.payload)] for o, p in zip(out_offs, pkts)])


def quic_seal(engine, pair, pkts, slots):
    """the packets sealed and header-protected under the pair's slots, as bytes per packet"""
    pkt_offs, pkt_total = place([p.pkt_len for p in pkts])
    in_offs, in_total = place([len(p.payload) for p in pkts])
    d_pkt = torch.from_numpy(image(pkt_total, pkt_offs, [p.header for p in pkts])).cuda()
    d_in = torch.from_numpy(image(in_total, in_offs, [p.payload for p in pkts])).cuda()
    q = ptls_hip.QuicBatch(engine, descriptors(pkts, pkt_offs, in_offs, slots, False), open=False)
    q.seal(pair[0], pair[1], d_in, d_pkt)
    torch.cuda.synchronize()
    q.close()
    out = d_pkt.cpu().numpy().tobytes()
    return [out[o: o + p.pkt_len] for o, p in zip(pkt_offs, pkts)]


def test_initial_sweep(engine):
    """65 connections into 130 slots from first = 2, every DCID length 0..20 at least three times, salts of both versions'
    length: the slots behave as Python's HKDF-Extract plus the reference's Expand-Label say, the slots around them keep
    their keys, packets quic_ref built under the client keys open on the client slots, and packets sealed on the server
    slots are quic_ref's bytes"""
    n, first = 65, 2
    dcids = [stream("dcid-%d" % i, i % 21) for i in range(n)]
    assert all(sum(len(d) == L for d in dcids) >= 3 for L in range(21))
    for labels, salt in ((1, kr.V1_SALT), (2, kr.V2_SALT)):
        pair = new_pair(engine, "aes128", first + 2 * n + 3)
        material = old_material("aes128", pair[0].nslots)
        load(pair, 0, material)
        pair[0].set_quic_initial(pair[1], first, dcids, salt, labels)
        for i, d in enumerate(dcids):
            material[first + 2 * i: first + 2 * i + 2] = [kr.keys(s, 16, labels == 2) for s in kr.initial_secrets(salt, d)]
        check_pair(engine, "aes128", pair, material, ("initial", labels))
        pkts = [Pkt(i, True) for i in range(n)]
        client, server = [first + 2 * i for i in range(n)], [first + 2 * i + 1 for i in range(n)]
        wire = [quic_ref.protect("aes128", *material[s], p.header, p.pn, p.payload) for s, p in zip(client, pkts)]
        res, pns, pts = quic_open(engine, pair, pkts, wire, client)
        assert res == [len(p.payload) for p in pkts] and pns == [p.pn for p in pkts] and pts == [p.payload for p in pkts], labels
        want = [quic_ref.protect("aes128", *material[s], p.header, p.pn, p.payload) for s, p in zip(server, pkts)]
        assert quic_seal(engine, pair, pkts, server) == want, labels
        close(pair)


A5_SECRET = bytes.fromhex("9ac312a7f877468ebe69422748ad00a15443f18203a07d6060f688f30f21632b")
A5_PACKET = bytes.fromhex("4cfe4189655e5cd55c41f69080575d7999c25a5bfb")
A5_NEXT = bytes.fromhex("1223504755036d556342ee9361d253421a826c9ecdf3c7148684b36b714881f9")


def test_rfc9001_a5_from_the_secret(engine):
    """RFC 9001 A.5 end to end from the secret alone: ChaCha keysets keyed by set_quic_secrets open the RFC's packet to
    payload 01 with packet number 654360564, and the key update returns the RFC's next secret"""
    pair = new_pair(engine, "chacha", 3)
    pair[0].set_quic_secrets(pair[1], 1, A5_SECRET, 32, 1)
    d = np.zeros(1, dtype=ptls_hip.QUIC_PACKET_DTYPE)
    d[0] = (5, 3, 654360564 - 1, len(A5_PACKET), 1, 1, 1, 0, 0)
    d_pkt = torch.from_numpy(image(64, [5], [A5_PACKET])).cuda()
    d_out = torch.full((16,), FILL, dtype=torch.uint8, device="cuda")
    d_res = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
    d_pn = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
    q = ptls_hip.QuicBatch(engine, d, open=True)
    q.open(pair[0], pair[1], d_pkt, d_out, d_res, d_pn)
    torch.cuda.synchronize()
    q.close()
    assert (int(d_res[0]), int(d_pn[0])) == (1, 654360564)
    assert np.array_equal(d_out.cpu().numpy(), image(16, [3], [b"\x01"]))
    assert np.array_equal(d_pkt.cpu().numpy(), image(64, [5], [bytes.fromhex("4200bff4") + A5_PACKET[4:]]))
    assert pair[0].update_quic_secrets(1, A5_SECRET, 32, 1) == A5_NEXT
    close(pair)


@pytest.mark.parametrize("algo", ["aes128", "aes256", "chacha"])
def test_key_update(engine, algo):
    """three generations over 65 connections (first = 1 of 67 slots): the returned secrets are the reference's "quic ku"
    chain; packets quic_ref built under generation g fail (UINT64_MAX, the packet number still decoded: header protection does
    not change) on the keyset after g - 1 updates and open on it after g; the slots around the range keep their keys; the
    masks from hp_ks are the same before and after"""
    _, ksz, hs = ALGOS[algo]
    n, first = 65, 1
    pair = new_pair(engine, algo, n + 2)
    material = old_material(algo, n + 2)
    load(pair, 0, material)
    secrets = [stream("ku-%s-%d" % (algo, i), hs) for i in range(n)]
    pair[0].set_quic_secrets(pair[1], first, b"".join(secrets), hs)
    material[first: first + n] = [kr.keys(s, ksz) for s in secrets]
    hp_keys = [m[2] for m in material]
    slots = list(range(first, first + n))
    masks_before = masks(engine, algo, pair[1], list(range(n + 2)))[0]
    pkts = [Pkt(i, False) for i in range(n)]
    lens, pns = [len(p.payload) for p in pkts], [p.pn for p in pkts]
    for g in (1, 2, 3):
        prev, secrets = secrets, [kr.update(s) for s in secrets]
        keys = [kr.keys(s, ksz) for s in secrets]
        wire = [quic_ref.protect(algo, k[0], k[1], hp_keys[s], p.header, p.pn, p.payload) for k, s, p in zip(keys, slots, pkts)]
        res, got_pns, _ = quic_open(engine, pair, pkts, wire, slots)
        assert res == [U64] * n and got_pns == pns, (algo, g, "before the update")
        got = pair[0].update_quic_secrets(first, b"".join(prev), hs)
        assert got == b"".join(secrets), (algo, g, "returned secrets")
        res, got_pns, pts = quic_open(engine, pair, pkts, wire, slots)
        assert res == lens and got_pns == pns and pts == [p.payload for p in pkts], (algo, g, "after the update")
        material[first: first + n] = [(k[0], k[1], hp) for k, hp in zip(keys, hp_keys[first: first + n])]
    check_pair(engine, algo, pair, material, (algo, "after three updates"))
    assert masks(engine, algo, pair[1], list(range(n + 2)))[0] == masks_before
    close(pair)


def test_refusals(engine):
    """every refusal of the three calls returns PTLS_HIP_EINVAL with its message and changes no slot: after each one the
    probe keysets behave as before; count == 0 returns 0"""
    L = ptls_hip.lib()
    pairs = {a: new_pair(engine, a, 8) for a in ALGOS}
    for a, pr in pairs.items():
        load(pr, 0, old_material(a, 8))
    small = new_pair(engine, "aes128", 4)
    load(small, 0, old_material("aes128", 4, "small"))
    other = ptls_hip.Engine(0)
    foreign = new_pair(other, "aes128", 8)
    load(foreign, 0, old_material("aes128", 8))
    before = {a: behaviour(engine, a, pr) for a, pr in pairs.items()}
    before_small = behaviour(engine, "aes128", small)
    k128, h128 = (k.ptr for k in pairs["aes128"])
    k256, h256 = (k.ptr for k in pairs["aes256"])
    kc, hc = (k.ptr for k in pairs["chacha"])
    sec = stream("refused", 8 * 48)
    dcids, lens, salt = stream("refused-dcid", 4 * 20), bytes([8, 0, 20, 5]), kr.V1_SALT

    def set_(ks=k128, hp=h128, first=0, count=4, s=sec, hs=32, labels=1):
        return L.ptls_hip_keyset_set_quic_secrets(ks, hp, first, count, s, hs, labels, None)

    def upd(ks=k128, first=0, count=4, s=sec, hs=32, labels=1):
        buf = None if s is None else ctypes.create_string_buffer(s, len(s))
        return L.ptls_hip_keyset_update_quic_secrets(ks, first, count, buf, hs, labels, None)

    def ini(ks=k128, hp=h128, first=0, count=4, d=dcids, ln=lens, sl=salt, slen=None, labels=1):
        return L.ptls_hip_keyset_set_quic_initial(ks, hp, first, count, d, ln, sl, len(salt) if slen is None else slen, labels, None)

    cases = [
        # a null pointer
        (lambda: set_(ks=None), "null keyset or secrets"), (lambda: set_(hp=None), "null keyset or secrets"),
        (lambda: set_(s=None), "null keyset or secrets"), (lambda: upd(ks=None), "null keyset or secrets"),
        (lambda: upd(s=None), "null keyset or secrets"), (lambda: ini(ks=None), "null keyset, connection IDs or salt"),
        (lambda: ini(hp=None), "null keyset, connection IDs or salt"), (lambda: ini(d=None), "null keyset, connection IDs or salt"),
        (lambda: ini(ln=None), "null keyset, connection IDs or salt"), (lambda: ini(sl=None), "null keyset, connection IDs or salt"),
        # a range past either keyset
        (lambda: set_(first=5), "lie past a keyset"), (lambda: set_(first=8, count=1), "lie past a keyset"),
        (lambda: set_(first=U64, count=2), "lie past a keyset"), (lambda: set_(hp=small[1].ptr, first=2), "lie past a keyset"),
        (lambda: set_(ks=small[0].ptr, first=2), "lie past a keyset"), (lambda: upd(first=5), "lie past a keyset"),
        (lambda: ini(first=1), "lie past a keyset"), (lambda: ini(first=0, count=5), "lie past a keyset"),
        (lambda: ini(hp=small[1].ptr, first=0, count=3), "lie past a keyset"),
        # count > 2^32 - 1
        (lambda: set_(count=1 << 32), "above 2^32 - 1"), (lambda: upd(count=1 << 32), "above 2^32 - 1"),
        (lambda: ini(count=1 << 32), "above 2^32 - 1"),
        # a hash_size that does not go with the keyset
        (lambda: set_(hs=48), "does not go with the keyset"), (lambda: upd(hs=48), "does not go with the keyset"),
        (lambda: set_(ks=kc, hp=hc, hs=48), "does not go with the keyset"), (lambda: upd(ks=kc, hs=48), "does not go with the keyset"),
        (lambda: set_(hs=20), "does not go with the keyset"), (lambda: set_(ks=k256, hp=h256, hs=64), "does not go with the keyset"),
        (lambda: upd(ks=k256, hs=0), "does not go with the keyset"),
        # labels other than 1 or 2
        (lambda: set_(labels=0), "labels must be"), (lambda: set_(labels=3), "labels must be"),
        (lambda: upd(labels=0), "labels must be"), (lambda: upd(labels=3), "labels must be"),
        (lambda: ini(labels=0), "labels must be"), (lambda: ini(labels=3), "labels must be"),
        # keysets of different engines, algorithms or key sizes
        (lambda: set_(hp=foreign[1].ptr), "differ in engine, algorithm or key size"),
        (lambda: ini(hp=foreign[1].ptr, count=2), "differ in engine, algorithm or key size"),
        (lambda: set_(hp=hc), "differ in engine, algorithm or key size"),
        (lambda: set_(ks=kc, hp=h256), "differ in engine, algorithm or key size"),
        (lambda: set_(hp=h256), "differ in engine, algorithm or key size"),
        (lambda: set_(ks=k256, hp=h128), "differ in engine, algorithm or key size"),
        (lambda: ini(hp=h256, count=2), "differ in engine, algorithm or key size"),
        # a connection ID longer than 20 bytes, a salt length outside 1..64
        (lambda: ini(ln=bytes([8, 0, 21, 5])), "dcid_lens[2] is 21"), (lambda: ini(ln=bytes([0, 0, 0, 255])), "dcid_lens[3] is 255"),
        (lambda: ini(slen=0), "outside 1..64"), (lambda: ini(sl=bytes(65), slen=65), "outside 1..64"),
        # the Initial call on anything but AES-128
        (lambda: ini(ks=k256, hp=h256), "Initial packets use AES-128-GCM"), (lambda: ini(ks=kc, hp=hc), "Initial packets use AES-128-GCM"),
        (lambda: ini(ks=k256, hp=h128), "Initial packets use AES-128-GCM"),
    ]
    for i, (call, msg) in enumerate(cases):
        assert call() == ptls_hip.EINVAL, (i, msg)
        assert msg in ptls_hip.last_error(), (i, msg, ptls_hip.last_error())
        torch.cuda.synchronize()
        for a, pr in pairs.items():
            assert behaviour(engine, a, pr) == before[a], (i, msg, a)
        assert behaviour(engine, "aes128", small) == before_small, (i, msg)
    # count == 0: nothing to do, whatever the first slot within the keysets
    assert set_(count=0) == 0 and set_(first=8, count=0) == 0 and upd(count=0) == 0 and ini(count=0) == 0 and ini(first=8, count=0) == 0
    for a, pr in pairs.items():
        assert behaviour(engine, a, pr) == before[a], a
    # the same objects, used as they are meant to be
    assert set_(first=4) == 0 and ini(first=0, count=2) == 0
    material = old_material("aes128", 8)
    material[4:8] = [kr.keys(sec[32 * i: 32 * i + 32], 16) for i in range(4)]
    for i in range(2):
        material[2 * i: 2 * i + 2] = [kr.keys(s, 16) for s in kr.initial_secrets(salt, dcids[20 * i: 20 * i + lens[i]])]
    check_pair(engine, "aes128", pairs["aes128"], material, "after the refusals")
    close(small, foreign, *pairs.values())
    other.close()
