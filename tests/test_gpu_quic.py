"""QUIC packet protection on the GPU (include/ptls_hip.h 2e; hsig-picotls_amd/csrc/quic_kernel.hip around the record kernels),
bit-exact against the plain-Python reference (tests/quic_ref.py: the CPU oracle for AES, tests/chacha_ref.py for ChaCha).
No tolerance anywhere: every comparison is a whole buffer against the reference's image of it.  Packets, payloads and
plaintexts lie at odd offsets with 1- to 64-byte gaps in 0xA5-filled buffers, result and pn_out start as a sentinel, so a
byte written outside a packet or a plaintext fails the test that wrote it.

Shapes: payloads of 0, 1, 2, 3 (with the packet-number lengths that still leave a header-protection sample inside the
packet), 15, 16, 17, 63, 64, 65, 255, 1200 and 1350 bytes under short headers with pn_offset 1, 9 and 21 and long headers with
pn_offset 18 and 47, every packet-number length with each, and one payload of 4000 bytes: 231 packets per case."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import ptls_hip
import quic_ref

pytestmark = pytest.mark.gpu
FILL = 0xA5
U64 = (1 << 64) - 1
SENTINEL = 0x5a5a5a5a5a5a5a5a
NKEYS = 64
PAYLOADS = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 1200, 1350]
HEADERS = [(0x40, 1), (0x40, 9), (0x40, 21), (0xc0, 18), (0xc0, 47)]  # (form and fixed bits, pn_offset)
ALGO_OF = {"aes128": (ptls_hip.ALGO_AESGCM, 16), "aes256": (ptls_hip.ALGO_AESGCM, 32),
           "chacha": (ptls_hip.ALGO_CHACHA20POLY1305, 32)}


def stream(tag, n):
    out, i = bytearray(), 0
    while len(out) < n:
        out += hashlib.sha256(b"%s/%d" % (tag.encode(), i)).digest()
        i += 1
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def key_material(algo):
    """(AEAD keys, static IVs, header-protection keys) of the NKEYS slots"""
    ksz = ALGO_OF[algo][1]
    return ([stream("gpu-quic-%s-key-%d" % (algo, i), ksz) for i in range(NKEYS)],
            [stream("gpu-quic-%s-iv-%d" % (algo, i), 12) for i in range(NKEYS)],
            [stream("gpu-quic-%s-hp-%d" % (algo, i), ksz) for i in range(NKEYS)])


PAYLOAD = stream("gpu-quic-payload", 8192)
HEADER = stream("gpu-quic-header", 4096)


@pytest.fixture(scope="module")
def keysets(engine):
    made = {}

    def get(algo):
        if algo not in made:
            kind, ksz = ALGO_OF[algo]
            keys, ivs, hps = key_material(algo)
            ks, hp = ptls_hip.KeySet(engine, ksz, NKEYS, algo=kind), ptls_hip.KeySet(engine, ksz, NKEYS, algo=kind)
            ks.set(0, b"".join(keys), b"".join(ivs))
            hp.set(0, b"".join(hps), None)
            made[algo] = (ks, hp)
        return made[algo]

    yield get
    torch.cuda.synchronize()
    for ks, hp in made.values():
        ks.close()
        hp.close()


class Spec:
    """one packet: key slots, the unprotected header (truncated packet number included), the packet number, the receiver's
    expected packet number, the payload"""

    def __init__(self, slot, hp_slot, header, pn_offset, pn, expected, payload):
        self.slot, self.hp_slot, self.header, self.pn_offset = slot, hp_slot, header, pn_offset
        self.pn, self.expected, self.payload = pn, expected, payload
        self.pn_len = len(header) - pn_offset
        assert self.pn_len == (header[0] & 3) + 1
        assert quic_ref.decode_pn(expected, int.from_bytes(header[pn_offset:], "big"), self.pn_len) == pn

    @property
    def pkt_len(self):
        return len(self.header) + len(self.payload) + 16


def pn_for(i, pn_len):
    """(packet number, the receiver's expected one): decodes that differ from the truncated value (the RFC 9000 A.3 example;
    0x1ff against 0x1fe in one byte), packet numbers >= 2^32 (the nonce's upper half) up to the last one below 2^62, 0, both
    far edges of the decode window, and truncated values that wrap around the window on either side of the expected one"""
    win = 1 << (8 * pn_len)
    h = win // 2
    if pn_len == 2 and i % 3 == 0:
        return 0xa82f9b32, 0xa82f30eb
    if pn_len == 1 and i % 3 == 0:
        return 0x1ff, 0x1fe
    k = i % 8
    if k == 0:
        return 0, 0
    if k == 1:
        return (1 << 32) + i * 977, (1 << 32) + i * 977 - 3
    if k == 2:
        return (1 << 62) - 1 - i, (1 << 62) - 1 - i - (h - 1)
    if k == 3:
        return i * 131 + 7, i * 131 + 7 + 5
    if k == 4:
        return (1 << 33) + win + 2, (1 << 33) + win - 3
    if k == 5:
        return (1 << 40) + win - 3, (1 << 40) + win + 3
    if k == 6:
        return (1 << 32) - 1, (1 << 32) - 1
    return 0xdeadbeefcafe + i + h - 1, 0xdeadbeefcafe + i


@functools.lru_cache(maxsize=None)
def shapes():
    out = []
    for L in PAYLOADS:
        for first, pn_offset in HEADERS:
            for pn_len in (1, 2, 3, 4):
                if pn_len + L >= 4:  # the sample at pn_offset + 4 ends inside the packet
                    out.append((first, pn_offset, pn_len, L))
    out.append((0x40, 9, 2, 4000))
    return out


@functools.lru_cache(maxsize=None)
def specs(mode):
    """the 231 shapes as packets.  mode "one": one AEAD key, lengths ascending (the plan's order is then not the caller's and
    the kernels read the plan-order descriptors); "runs": three keys, 77 packets each, ascending; "many": packet i under key
    i % 64 in shape order (one packet per key run: the wave-per-record AES kernel)."""
    sh = list(shapes())
    if mode != "many":
        sh.sort(key=lambda s: s[3])
    n, out = len(sh), []
    for i, (first, pn_offset, pn_len, L) in enumerate(sh):
        slot = 0 if mode == "one" else (7, 0, 63)[i * 3 // n] if mode == "runs" else i % NKEYS
        pn, expected = pn_for(i, pn_len)
        # every protected bit of the first byte varies: reserved bits / key phase (short), type and reserved bits (long)
        fb = first | ((i * 4) & 0x3c) | (pn_len - 1)
        header = bytes([fb]) + HEADER[i: i + pn_offset - 1] + (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big")
        out.append(Spec(slot, (i * 5 + 1) % NKEYS, header, pn_offset, pn, expected, PAYLOAD[i: i + L]))
    return out


@functools.lru_cache(maxsize=None)
def ref_protect(algo, slot, hp_slot, header, pn, payload):
    keys, ivs, hps = key_material(algo)
    return quic_ref.protect(algo, keys[slot], ivs[slot], hps[hp_slot], header, pn, payload)


def protected(algo, sp):
    return [ref_protect(algo, s.slot, s.hp_slot, s.header, s.pn, s.payload) for s in sp]


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


def dev(buf):
    return torch.from_numpy(buf).cuda()


def descriptors(sp, pkt_offs, data_offs, is_open, flags=0, slots=None):
    d = np.zeros(len(sp), dtype=ptls_hip.QUIC_PACKET_DTYPE)
    d["pkt_off"], d["data_off"] = pkt_offs, data_offs
    d["pn"] = [s.expected if is_open else s.pn for s in sp]
    d["pkt_len"] = [s.pkt_len for s in sp]
    d["key"] = [s.slot for s in sp] if slots is None else slots
    d["hp_key"] = [s.hp_slot for s in sp]
    d["pn_offset"] = [s.pn_offset for s in sp]
    d["pn_len"] = [9 if is_open else s.pn_len for s in sp]  # open ignores it
    d["flags"] = flags
    return d


def set_lanes(q, algo, lanes):
    b = q.records()
    if lanes:
        if algo == "chacha":
            b.set_chacha_lanes(lanes)
            assert b.chacha_lanes == lanes
        else:
            b.set_lanes(lanes)
            assert b.lanes == lanes
    return b


def check_seal(engine, keysets, algo, sp, lanes, in_place):
    ks, hp = keysets(algo)
    pkt_offs, pkt_total = place([s.pkt_len for s in sp])
    h_pkt = image(pkt_total, pkt_offs, [s.header for s in sp])  # the caller has written the unprotected headers
    if in_place:
        data_offs = [o + len(s.header) for o, s in zip(pkt_offs, sp)]
        h_pkt = image(pkt_total, pkt_offs, [s.header + s.payload for s in sp])
        d_pkt = d_in = dev(h_pkt)
        h_in = None
    else:
        data_offs, in_total = place([len(s.payload) for s in sp])
        h_in = image(in_total, data_offs, [s.payload for s in sp])
        d_pkt, d_in = dev(h_pkt), dev(h_in)
    q = ptls_hip.QuicBatch(engine, descriptors(sp, pkt_offs, data_offs, False), open=False)
    set_lanes(q, algo, lanes)
    q.seal(ks, hp, d_in, d_pkt)
    torch.cuda.synchronize()
    q.close()
    assert np.array_equal(d_pkt.cpu().numpy(), image(pkt_total, pkt_offs, protected(algo, sp))), ("seal", algo, lanes, in_place)
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy(), h_in)


def run_open(engine, keysets, algo, sp, lanes, packets, flags=0, slots=None, want_lanes=None):
    """one open call over `packets` (bytes per packet, as received); returns (result, pn_out, pkt after, out, layout)"""
    ks, hp = keysets(algo)
    pkt_offs, pkt_total = place([s.pkt_len for s in sp])
    out_offs, out_total = place([len(s.payload) + 4 for s in sp])  # (a damaged pn_len makes a payload up to 3 bytes longer)
    d_pkt = dev(image(pkt_total, pkt_offs, packets))
    d_out = dev(np.full(out_total, FILL, np.uint8))
    d_res = torch.full((len(sp),), SENTINEL, dtype=torch.int64, device="cuda")
    d_pn = torch.full((len(sp),), SENTINEL, dtype=torch.int64, device="cuda")
    q = ptls_hip.QuicBatch(engine, descriptors(sp, pkt_offs, out_offs, True, flags, slots), open=True)
    b = set_lanes(q, algo, lanes)
    if want_lanes is not None:
        assert b.lanes == want_lanes
    q.open(ks, hp, d_pkt, d_out, d_res, d_pn)
    torch.cuda.synchronize()
    q.close()
    res = [int(x) & U64 for x in d_res.cpu().numpy().tolist()]
    pns = [int(x) & U64 for x in d_pn.cpu().numpy().tolist()]
    return res, pns, d_pkt.cpu().numpy(), d_out.cpu().numpy(), (pkt_offs, pkt_total, out_offs, out_total)


def check_open(engine, keysets, algo, sp, lanes, want_lanes=None):
    packets = protected(algo, sp)
    res, pns, pkt, out, (pkt_offs, pkt_total, out_offs, out_total) = run_open(engine, keysets, algo, sp, lanes, packets,
                                                                              want_lanes=want_lanes)
    assert pns == [s.pn for s in sp], ("pn_out", algo, lanes)
    assert res == [len(s.payload) for s in sp], ("result", algo, lanes)
    # the headers come back unprotected, nothing else in pkt changes
    want_pkt = [s.header + p[len(s.header):] for s, p in zip(sp, packets)]
    assert np.array_equal(pkt, image(pkt_total, pkt_offs, want_pkt)), ("pkt", algo, lanes)
    assert np.array_equal(out, image(out_total, out_offs, [s.payload for s in sp])), ("out", algo, lanes)


@pytest.mark.parametrize("lanes", [1, 4, 32])
@pytest.mark.parametrize("algo", ["aes128", "aes256"])
def test_aes_one_key(engine, keysets, algo, lanes):
    """231 packets under one key in ascending length, lanes per record forced: the batch kernel, plan order != caller order"""
    sp = specs("one")
    check_seal(engine, keysets, algo, sp, lanes, False)
    check_seal(engine, keysets, algo, sp, lanes, True)
    check_open(engine, keysets, algo, sp, lanes)


def test_aes256_one_packet_per_key(engine, keysets):
    """one packet per key run over 64 keys: the planner picks the wave-per-record kernel (lanes 64)"""
    sp = specs("many")
    check_seal(engine, keysets, "aes256", sp, 0, False)
    check_seal(engine, keysets, "aes256", sp, 0, True)
    check_open(engine, keysets, "aes256", sp, 0, want_lanes=64)


@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_chacha_many_keys(engine, keysets, lanes):
    sp = specs("many")
    check_seal(engine, keysets, "chacha", sp, lanes, False)
    check_seal(engine, keysets, "chacha", sp, lanes, True)
    check_open(engine, keysets, "chacha", sp, lanes)


def test_rfc9001_a5_packet(engine):
    """the ChaCha20-Poly1305 short-header packet of RFC 9001 A.5 seals and opens to the RFC's exact bytes (its sample is its
    whole tag and ends with the packet: pkt_len == pn_offset + 20)"""
    key = bytes.fromhex("c6d98ff3441c3fe1b2182094f69caa2ed4b716b65488960a7a984979fb23e1c8")
    iv = bytes.fromhex("e0459b3474bdd0e44a41c144")
    hpk = bytes.fromhex("25a282b9e82f06f21f488917a4fc8f1b73573685608597d0efcb076b0ab7a7a4")
    header, payload, pn = bytes.fromhex("4200bff4"), bytes.fromhex("01"), 654360564
    packet = bytes.fromhex("4cfe4189655e5cd55c41f69080575d7999c25a5bfb")
    assert quic_ref.protect("chacha", key, iv, hpk, header, pn, payload) == packet
    ks = ptls_hip.KeySet(engine, 32, 3, algo=ptls_hip.ALGO_CHACHA20POLY1305)
    hp = ptls_hip.KeySet(engine, 32, 2, algo=ptls_hip.ALGO_CHACHA20POLY1305)
    ks.set(2, key, iv)
    hp.set(1, hpk, None)
    d = np.zeros(1, dtype=ptls_hip.QUIC_PACKET_DTYPE)
    d[0] = (7, 3, pn, len(packet), 2, 1, 1, 3, 0)
    d_pkt = dev(image(64, [7], [header]))
    d_in = dev(image(16, [3], [payload]))
    q = ptls_hip.QuicBatch(engine, d, open=False)
    q.seal(ks, hp, d_in, d_pkt)
    torch.cuda.synchronize()
    q.close()
    assert np.array_equal(d_pkt.cpu().numpy(), image(64, [7], [packet]))
    d["pn"], d["pn_len"] = pn - 1, 0  # the receiver expects the packet before it
    d_out = dev(np.full(16, FILL, np.uint8))
    d_res = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
    d_pn = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
    q = ptls_hip.QuicBatch(engine, d, open=True)
    q.open(ks, hp, d_pkt, d_out, d_res, d_pn)
    torch.cuda.synchronize()
    q.close()
    assert (int(d_res[0]), int(d_pn[0])) == (1, pn)
    assert np.array_equal(d_pkt.cpu().numpy(), image(64, [7], [header + packet[4:]]))
    assert np.array_equal(d_out.cpu().numpy(), image(16, [3], [payload]))
    ks.close()
    hp.close()


def flip(pkt, pos, bit):
    b = bytearray(pkt)
    b[pos] ^= 1 << bit
    return bytes(b)


@pytest.mark.parametrize("algo", ["aes128", "aes256", "chacha"])
def test_damaged_packet(engine, keysets, algo):
    """one packet in the middle of a batch with one flipped bit, in turn in the payload, the tag, a protected packet-number
    byte, each of the low two bits of the first byte (the packet-number length changes) and the sample: that packet's result
    is UINT64_MAX and its header, pn_out and plaintext bytes are what the reference computes for the damaged packet; every
    other packet and every gap byte is untouched"""
    sp = [s for s in specs("runs") if len(s.payload) >= 15][::3]
    j = next(i for i in range(len(sp) // 2, len(sp)) if sp[i].pn_len == 2 and len(sp[i].payload) >= 63)
    s = sp[j]
    hl = len(s.header)
    keys, ivs, hps = key_material(algo)
    good = protected(algo, sp)
    damages = {"payload": (hl + 40, 3), "tag": (s.pkt_len - 1, 7), "pn byte": (s.pn_offset + 1, 0),
               "first byte bit 0": (0, 0), "first byte bit 1": (0, 1), "sample": (s.pn_offset + 4 + 9, 5)}
    for kind, (pos, bit) in damages.items():
        packets = list(good)
        packets[j] = flip(good[j], pos, bit)
        header, pn, pt, ok = quic_ref.unprotect(algo, keys[s.slot], ivs[s.slot], hps[s.hp_slot], packets[j], s.pn_offset,
                                                s.expected)
        assert not ok, kind
        if kind.startswith("first"):
            assert len(header) != hl and len(pt) != len(s.payload)
        res, pns, pkt, out, (pkt_offs, pkt_total, out_offs, out_total) = run_open(engine, keysets, algo, sp, 0, packets)
        assert res == [U64 if i == j else len(x.payload) for i, x in enumerate(sp)], kind
        assert pns == [pn if i == j else x.pn for i, x in enumerate(sp)], kind
        want_pkt = [x.header + p[len(x.header):] for x, p in zip(sp, packets)]
        want_pkt[j] = header + packets[j][len(header):]
        assert np.array_equal(pkt, image(pkt_total, pkt_offs, want_pkt)), kind
        want_out = [x.payload for x in sp]
        want_out[j] = pt
        assert np.array_equal(out, image(out_total, out_offs, want_out)), kind


@pytest.mark.parametrize("algo", ["aes128", "aes256", "chacha"])
def test_unprotected_flag_and_second_key(engine, keysets, algo):
    """opening the already-opened packets again with PTLS_HIP_QUIC_UNPROTECTED gives the same results and changes no byte of
    pkt; a packet sealed under key B fails under key A and then opens under key B with the flag"""
    sp = specs("runs")[::4]
    j = len(sp) // 2
    key_b, key_a = sp[j].slot, 33
    ks, hp = keysets(algo)
    keys, ivs, hps = key_material(algo)
    packets = protected(algo, sp)
    pkt_offs, pkt_total = place([s.pkt_len for s in sp])
    out_offs, out_total = place([len(s.payload) + 4 for s in sp])
    d_pkt = dev(image(pkt_total, pkt_offs, packets))
    want_pkt = image(pkt_total, pkt_offs, [s.header + p[len(s.header):] for s, p in zip(sp, packets)])
    lens, pns = [len(s.payload) for s in sp], [s.pn for s in sp]
    slots_a = [key_a if i == j else s.slot for i, s in enumerate(sp)]
    wrong_pt, ok = quic_ref.aead_open(algo, keys[key_a], ivs[key_a], sp[j].pn, sp[j].header, packets[j][len(sp[j].header):])
    assert not ok
    steps = [(0, slots_a, [U64 if i == j else l for i, l in enumerate(lens)], [wrong_pt if i == j else s.payload
                                                                             for i, s in enumerate(sp)]),
             (ptls_hip.QUIC_UNPROTECTED, None, lens, [s.payload for s in sp]),
             (ptls_hip.QUIC_UNPROTECTED, None, lens, [s.payload for s in sp])]
    assert key_a != key_b
    for flags, slots, want_res, want_pt in steps:
        d_out = dev(np.full(out_total, FILL, np.uint8))
        d_res = torch.full((len(sp),), SENTINEL, dtype=torch.int64, device="cuda")
        d_pn = torch.full((len(sp),), SENTINEL, dtype=torch.int64, device="cuda")
        q = ptls_hip.QuicBatch(engine, descriptors(sp, pkt_offs, out_offs, True, flags, slots), open=True)
        q.open(ks, hp, d_pkt, d_out, d_res, d_pn)
        torch.cuda.synchronize()
        q.close()
        assert [int(x) & U64 for x in d_res.cpu().numpy().tolist()] == want_res, flags
        assert [int(x) & U64 for x in d_pn.cpu().numpy().tolist()] == pns, flags
        assert np.array_equal(d_pkt.cpu().numpy(), want_pkt), flags
        assert np.array_equal(d_out.cpu().numpy(), image(out_total, out_offs, want_pt)), flags


def test_refusals(engine, keysets):
    """every refusal returns NULL / PTLS_HIP_EINVAL with the packet's index in the message, all buffers stay at their fill,
    and a correct call on the same objects then passes; n == 0 succeeds and launches nothing"""
    L = ptls_hip.lib()
    sp = specs("runs")[::16]
    n = len(sp)
    pkt_offs, pkt_total = place([s.pkt_len for s in sp])
    data_offs, data_total = place([len(s.payload) + 4 for s in sp])
    good_seal = descriptors(sp, pkt_offs, data_offs, False)
    good_open = descriptors(sp, pkt_offs, data_offs, True)
    # refused when the batch is made
    for is_open, field, value, msg in ((0, "pn_offset", 0, "pn_offset is 0"), (1, "pn_offset", 0, "pn_offset is 0"),
                                       (0, "pn_len", 0, "pn_len must be 1..4"), (0, "pn_len", 5, "pn_len must be 1..4"),
                                       (0, "pn", 1 << 62, "below 2^62"),
                                       (0, "pkt_len", None, "pkt_len < pn_offset + 20"),
                                       (1, "pkt_len", None, "pkt_len < pn_offset + 20")):
        d = (good_open if is_open else good_seal).copy()
        d[field][n - 2] = d["pn_offset"][n - 2] + 19 if value is None else value
        assert L.ptls_hip_quic_batch_new(engine.ptr, d.ctypes.data, n, is_open, None) is None, (field, value)
        err = ptls_hip.last_error()
        assert "packet %d:" % (n - 2) in err and msg in err, err
    # refused at the call
    ks, hp = keysets("aes128")
    ks256, hp256 = keysets("aes256")
    ksc, hpc = keysets("chacha")
    small = ptls_hip.KeySet(engine, 16, 4)
    d_in = dev(image(data_total, data_offs, [s.payload for s in sp]))
    h_pkt = image(pkt_total, pkt_offs, [s.header for s in sp])
    d_pkt = dev(h_pkt)
    d_out = dev(np.full(data_total, FILL, np.uint8))
    d_res = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda")
    d_pn = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda")
    qs = ptls_hip.QuicBatch(engine, good_seal, open=False)
    qo = ptls_hip.QuicBatch(engine, good_open, open=True)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    k = max(range(n), key=lambda i: sp[i].slot)
    kh = max(range(n), key=lambda i: sp[i].hp_slot)
    assert sp[k].slot >= 4 and sp[kh].hp_slot >= 4

    def seal(q=qs, a=ks, h=hp, i=d_in, pk=d_pkt):
        return L.ptls_hip_quic_seal_batch(q.ptr, a.ptr, h.ptr, p(i), p(pk), None)

    def open_(q=qo, a=ks, h=hp, pk=d_pkt, o=d_out, r=d_res, pn=d_pn):
        return L.ptls_hip_quic_open_batch(q.ptr, a.ptr, h.ptr, p(pk), p(o), p(r), p(pn), None)

    calls = [
        (lambda: seal(a=small), "packet %d names key slot" % k),
        (lambda: open_(a=small), "packet %d names key slot" % k),
        (lambda: seal(h=small), "packet %d names header-protection key slot" % kh),
        (lambda: open_(h=small), "packet %d names header-protection key slot" % kh),
        (lambda: seal(h=hp256), "algorithm and key size"),
        (lambda: open_(h=hp256), "algorithm and key size"),
        (lambda: seal(a=ks256), "algorithm and key size"),
        (lambda: seal(h=hpc), "algorithm and key size"),
        (lambda: open_(a=ksc), "algorithm and key size"),
        (lambda: seal(q=qo), "the batch was made for open"),
        (lambda: open_(q=qs), "the batch was made for seal"),
        (lambda: seal(i=None), "null buffer"),
        (lambda: seal(pk=None), "null buffer"),
        (lambda: open_(pk=None), "null buffer"),
        (lambda: open_(o=None), "null buffer"),
        (lambda: open_(r=None), "null buffer"),
        (lambda: open_(pn=None), "null buffer"),
    ]
    for call, msg in calls:
        assert call() == ptls_hip.EINVAL, msg
        assert msg in ptls_hip.last_error(), (msg, ptls_hip.last_error())
    torch.cuda.synchronize()
    assert np.array_equal(d_pkt.cpu().numpy(), h_pkt)
    assert bool((d_out == FILL).all()) and bool((d_res == SENTINEL).all()) and bool((d_pn == SENTINEL).all())
    # n == 0: both calls succeed, whatever the buffers
    for is_open in (0, 1):
        q0 = L.ptls_hip_quic_batch_new(engine.ptr, None, 0, is_open, None)
        assert q0
        if is_open:
            assert L.ptls_hip_quic_open_batch(q0, ks.ptr, hp.ptr, None, None, None, None, None) == 0
        else:
            assert L.ptls_hip_quic_seal_batch(q0, ks.ptr, hp.ptr, None, None, None) == 0
        L.ptls_hip_quic_batch_free(q0)
    torch.cuda.synchronize()
    assert np.array_equal(d_pkt.cpu().numpy(), h_pkt)
    # the same objects, used as they are meant to be
    assert seal() == 0
    assert open_() == 0
    torch.cuda.synchronize()
    packets = protected("aes128", sp)
    assert np.array_equal(d_pkt.cpu().numpy(), image(pkt_total, pkt_offs, [s.header + x[len(s.header):]
                                                                            for s, x in zip(sp, packets)]))
    assert np.array_equal(d_out.cpu().numpy(), image(data_total, data_offs, [s.payload for s in sp]))
    assert [int(x) & U64 for x in d_res.cpu().numpy().tolist()] == [len(s.payload) for s in sp]
    assert [int(x) & U64 for x in d_pn.cpu().numpy().tolist()] == [s.pn for s in sp]
    qs.close()
    qo.close()
    small.close()
