"""QUIC packet protection from and to host memory (include/ptls_hip.h 2g: ptls_hip_pipeline_quic_seal / _open), bit-exact
against the plain-Python reference (tests/quic_ref.py).  No tolerance anywhere: every comparison is a WHOLE caller buffer
against its expected image, the position-dependent prefill (mask_prefill) with the reference's bytes laid in, so a byte
written outside a packet, a header or a plaintext fails the test that wrote it, and so does a right byte at a wrong place.
Packets, payloads and plaintext areas lie at odd offsets 1 to 64 bytes apart; a plaintext area has the pn_len = 1 size
(pkt_len - pn_offset - 17), up to 3 bytes more than its plaintext; result and pn_out start as sentinels.  64 KiB slices, the
minimum, so the 924 packets of the main matrix (more than 4 x 64 KiB) are cut into at least five slices on the copy
transport and every slot is reused while others are in flight."""
import functools

import numpy as np
import pytest
import torch

import ptls_hip
import quic_keys_ref as kr
import quic_ref
from test_gpu_copy_gaps import Bufs, _same, image, mask_prefill
from test_gpu_quic import (ALGO_OF, HEADER, NKEYS, PAYLOAD, SENTINEL, U64, Spec, descriptors, flip, key_material, keysets,  # noqa: F401
                           place, protected, specs, stream)

pytestmark = pytest.mark.gpu
COPY, MAPPED, AUTO = ptls_hip.TRANSPORT_COPY, ptls_hip.TRANSPORT_MAPPED, ptls_hip.TRANSPORT_AUTO
SLICE = 64 << 10
CIPHERS = [("aes128", "one"), ("aes256", "many"), ("chacha", "many")]
TRANSPORTS = [(COPY, "pageable"), (COPY, "pinned"), (MAPPED, "pinned")]


@functools.lru_cache(maxsize=None)
def packets(mode):
    """the 231 shapes of test_gpu_quic.specs(mode) four times, key slots and packet numbers shifted per repetition"""
    out = []
    for rep in range(4):
        for s in specs(mode):
            delta = rep * 0x10101
            if s.pn + delta >= 1 << 62 or s.expected + delta >= 1 << 62:
                delta = -delta
            pn, expected = s.pn + delta, s.expected + delta
            header = s.header[:s.pn_offset] + (pn & ((1 << (8 * s.pn_len)) - 1)).to_bytes(s.pn_len, "big")
            out.append(Spec((s.slot + 17 * rep) % NKEYS, (s.hp_slot + 3 * rep) % NKEYS, header, s.pn_offset, pn, expected, s.payload))
    assert len(out) == 924 and sum(s.pkt_len for s in out) > 4 * SLICE
    return out


def area(s):
    """the plaintext area of a packet: the pn_len = 1 size, which is all the caller can know"""
    return s.pkt_len - s.pn_offset - 17


def pipeline(engine, algo, transport):
    return ptls_hip.Pipeline(engine, SLICE, transport=transport, algo=ALGO_OF[algo][0])


def sentinels(bufs, n):
    return bufs(np.full(n, SENTINEL, np.uint64))


def ints(a):
    return [int(x) for x in a]


def check_seal(pipe, keys, sp, sealed, perm, kind, transport, in_place):
    """one seal call: the whole h_pkt (and h_in) against their images"""
    ks, hp = keys
    bufs = Bufs(kind)
    pkt_offs, pkt_total = place([s.pkt_len for s in sp])
    base = mask_prefill(pkt_total)
    if in_place:
        data_offs = [o + len(s.header) for o, s in zip(pkt_offs, sp)]
        h_pkt = h_in = bufs(image(base, pkt_offs, [s.header + s.payload for s in sp]))
    else:
        data_offs, in_total = place([len(s.payload) for s in sp])
        in_img = image(mask_prefill(in_total), data_offs, [s.payload for s in sp])
        h_pkt, h_in = bufs(image(base, pkt_offs, [s.header for s in sp])), bufs(in_img)  # the caller wrote the headers
    pipe.quic_seal(ks, hp, descriptors(sp, pkt_offs, data_offs, False)[perm], h_in, h_pkt)
    assert pipe.last_transport == transport
    _same(h_pkt, image(base, pkt_offs, sealed), "seal h_pkt (in place: %s)" % in_place)
    if not in_place:
        _same(h_in, in_img, "seal wrote h_in")


def check_open(pipe, keys, sp, received, want, perm, kind, transport, flags=0, slots=None, res_kind=None, pkt_after=None):
    """one open call over the packets `received`; want[i] = (header, pn, plaintext, ok) of packet i.  The whole h_pkt, the
    whole h_out, result and pn_out against their images.  Returns the h_pkt image after the call."""
    ks, hp = keys
    bufs, rbufs = Bufs(kind), Bufs(res_kind or kind)
    n = len(sp)
    pkt_offs, pkt_total = place([s.pkt_len for s in sp])
    out_offs, out_total = place([area(s) for s in sp])
    pkt_base, out_base = mask_prefill(pkt_total), mask_prefill(out_total)
    h_pkt, h_out = bufs(image(pkt_base, pkt_offs, received)), bufs(out_base)
    h_res, h_pn = sentinels(rbufs, n), sentinels(rbufs, n)
    pipe.quic_open(ks, hp, descriptors(sp, pkt_offs, out_offs, True, flags, slots)[perm], h_pkt, h_out, h_res, h_pn)
    assert pipe.last_transport == transport
    if pkt_after is None:  # the headers come back unprotected, nothing else in h_pkt changes
        pkt_after = [w[0] + r[len(w[0]):] for w, r in zip(want, received)]
    _same(h_pkt, image(pkt_base, pkt_offs, pkt_after), "open h_pkt")
    _same(h_out, image(out_base, out_offs, [w[2] for w in want]), "open h_out")
    assert ints(h_res) == [len(want[i][2]) if want[i][3] else U64 for i in perm], "result"
    assert ints(h_pn) == [want[i][1] for i in perm], "pn_out"
    return pkt_after


def good(sp):
    return [(s.header, s.pn, s.payload, True) for s in sp]


def order(n, shuffled, seed=7):
    return np.random.default_rng(seed).permutation(n) if shuffled else np.arange(n)


@pytest.mark.parametrize("shuffled", [False, True], ids=["in_order", "shuffled"])
@pytest.mark.parametrize("transport,kind", TRANSPORTS, ids=["copy-pageable", "copy-pinned", "mapped-pinned"])
@pytest.mark.parametrize("algo,mode", CIPHERS, ids=[c[0] for c in CIPHERS])
def test_main_matrix(engine, keysets, algo, mode, transport, kind, shuffled):
    """924 packets: seal not in place, seal in place, then open on the pipeline that has just sealed (its staging holds
    foreign bytes)"""
    sp = packets(mode)
    sealed = protected(algo, sp)
    perm = order(len(sp), shuffled)
    pipe = pipeline(engine, algo, transport)
    try:
        check_seal(pipe, keysets(algo), sp, sealed, perm, kind, transport, False)
        check_seal(pipe, keysets(algo), sp, sealed, perm, kind, transport, True)
        check_open(pipe, keysets(algo), sp, sealed, good(sp), perm, kind, transport)
    finally:
        pipe.close()


def test_auto_transport(engine, keysets):
    """AUTO: pageable buffers take COPY, pinned ones MAPPED, and pinned packets with pageable h_result / h_pn_out still
    MAPPED, both arrays travelling through the slot"""
    sp = specs("runs")[::2]
    sealed = protected("aes128", sp)
    perm = order(len(sp), False)
    pipe = pipeline(engine, "aes128", AUTO)
    try:
        for kind, transport, res_kind in (("pageable", COPY, None), ("pinned", MAPPED, None), ("pinned", MAPPED, "pageable")):
            check_seal(pipe, keysets("aes128"), sp, sealed, perm, kind, transport, False)
            check_open(pipe, keysets("aes128"), sp, sealed, good(sp), perm, kind, transport, res_kind=res_kind)
    finally:
        pipe.close()


@functools.lru_cache(maxsize=None)
def tiny_packets():
    """1 100 packets of 21 to 24 bytes under pn_offset 1: payloads of 0 to 3 bytes with the packet-number lengths that keep
    the header-protection sample inside the packet (pn_len + payload >= 4)"""
    shapes = [(pn_len, L) for pn_len in (1, 2, 3, 4) for L in (0, 1, 2, 3) if pn_len + L >= 4]
    out = []
    for i in range(1100):
        pn_len, L = shapes[i % len(shapes)]
        pn = 5000 + 3 * i
        header = bytes([0x40 | ((i * 4) & 0x3c) | (pn_len - 1)]) + (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big")
        out.append(Spec(i % NKEYS, (i * 5 + 1) % NKEYS, header, 1, pn, pn - 1, PAYLOAD[i: i + L]))
    assert all(21 <= s.pkt_len <= 24 for s in out) and len(out) > SLICE // 64
    return out


@pytest.mark.parametrize("kind", ["pinned", "pageable"])
def test_packet_cap(engine, keysets, kind):
    """more packets than a slice may hold (64 KiB / 64 = 1 024) inside one slice's span: the copy transport cuts at the cap"""
    sp = tiny_packets()
    sealed = protected("aes128", sp)
    perm = order(len(sp), False)
    pipe = pipeline(engine, "aes128", COPY)
    try:
        check_seal(pipe, keysets("aes128"), sp, sealed, perm, kind, COPY, False)
        check_seal(pipe, keysets("aes128"), sp, sealed, perm, kind, COPY, True)
        check_open(pipe, keysets("aes128"), sp, sealed, good(sp), perm, kind, COPY)
    finally:
        pipe.close()


@pytest.mark.parametrize("algo,mode", CIPHERS, ids=[c[0] for c in CIPHERS])
def test_damaged_packets_on_copy(engine, keysets, algo, mode):
    """the damages of test_gpu_quic.test_damaged_packet -- payload, tag, a packet-number byte, each of the two low bits of the
    first byte (pn_len and with it the plaintext length change by up to 3), the sample -- in three packets that lie in three
    different slices: the whole h_out equals the reference's image, the bytes of each area behind its plaintext included;
    h_pkt, result and pn_out are what quic_ref.unprotect gives"""
    sp = packets(mode)
    sealed = protected(algo, sp)
    keys, ivs, hps = key_material(algo)
    pkt_offs, _ = place([s.pkt_len for s in sp])
    victims = []
    for lo in (60, 400, 780):
        victims.append(next(i for i in range(lo, len(sp)) if sp[i].pn_len == 2 and len(sp[i].payload) >= 63))
    # in order, a slice's packets span at most 64 KiB: packets further apart than that lie in different slices
    assert all(pkt_offs[b] - pkt_offs[a] > SLICE for a, b in zip(victims, victims[1:]))
    pipe = pipeline(engine, algo, COPY)
    try:
        for kind in ("payload", "tag", "pn byte", "first byte bit 0", "first byte bit 1", "sample"):
            received, want = list(sealed), good(sp)
            for j in victims:
                s = sp[j]
                pos, bit = {"payload": (len(s.header) + 40, 3), "tag": (s.pkt_len - 1, 7), "pn byte": (s.pn_offset + 1, 0),
                            "first byte bit 0": (0, 0), "first byte bit 1": (0, 1), "sample": (s.pn_offset + 4 + 9, 5)}[kind]
                received[j] = flip(sealed[j], pos, bit)
                want[j] = quic_ref.unprotect(algo, keys[s.slot], ivs[s.slot], hps[s.hp_slot], received[j], s.pn_offset, s.expected)
                assert not want[j][3], kind
                if kind.startswith("first"):
                    assert len(want[j][0]) != len(s.header) and len(want[j][2]) != len(s.payload) and len(want[j][2]) <= area(s)
            check_open(pipe, keysets(algo), sp, received, want, order(len(sp), False), "pinned", COPY)
    finally:
        pipe.close()


@pytest.mark.parametrize("transport,kind", [(COPY, "pinned"), (MAPPED, "pinned")], ids=["copy", "mapped"])
@pytest.mark.parametrize("algo", ["aes128", "aes256", "chacha"])
def test_unprotected_flag_and_second_key(engine, keysets, algo, transport, kind):
    """a packet sealed under key B fails under key A; then, its header being unprotected already, it opens under key B with
    PTLS_HIP_QUIC_UNPROTECTED; reopening everything with the flag changes no byte of h_pkt and gives the same results"""
    sp = specs("runs")[::4]
    j = len(sp) // 2
    key_a = 33
    assert sp[j].slot != key_a
    keys, ivs, _ = key_material(algo)
    sealed = protected(algo, sp)
    wrong_pt, ok = quic_ref.aead_open(algo, keys[key_a], ivs[key_a], sp[j].pn, sp[j].header, sealed[j][len(sp[j].header):])
    assert not ok
    under_a = good(sp)
    under_a[j] = (sp[j].header, sp[j].pn, wrong_pt, False)
    perm = order(len(sp), True)
    pipe = pipeline(engine, algo, transport)
    try:
        opened = check_open(pipe, keysets(algo), sp, sealed, under_a, perm, kind, transport,
                            slots=[key_a if i == j else s.slot for i, s in enumerate(sp)])
        for _ in range(2):
            check_open(pipe, keysets(algo), sp, opened, good(sp), perm, kind, transport, flags=ptls_hip.QUIC_UNPROTECTED,
                       pkt_after=opened)
    finally:
        pipe.close()


@pytest.mark.parametrize("transport,kind", [(COPY, "pageable"), (MAPPED, "pinned")], ids=["copy", "mapped"])
@pytest.mark.parametrize("algo", ["aes128", "chacha"])
def test_keys_that_exist_only_on_the_device(engine, algo, transport, kind):
    """keysets filled by set_quic_secrets (8 connections; the header-protection keys never exist on the host side of the
    library) seal and open host-resident packets; the expected bytes come from tests/quic_keys_ref.py and quic_ref.py"""
    kind_, ksz = ALGO_OF[algo]
    secrets = [stream("quic-pipeline-secret-%s-%d" % (algo, c), 32) for c in range(8)]
    ks, hp = ptls_hip.KeySet(engine, ksz, 10, algo=kind_), ptls_hip.KeySet(engine, ksz, 10, algo=kind_)
    ks.set_quic_secrets(hp, 1, b"".join(secrets), 32)
    material = [kr.keys(s, ksz) for s in secrets]
    sp = [Spec(1 + i % 8, 1 + i % 8, s.header, s.pn_offset, s.pn, s.expected, s.payload) for i, s in enumerate(specs("many")[::3])]
    sealed = [quic_ref.protect(algo, *material[s.slot - 1], s.header, s.pn, s.payload) for s in sp]
    pipe = pipeline(engine, algo, transport)
    try:
        perm = order(len(sp), True)
        check_seal(pipe, (ks, hp), sp, sealed, perm, kind, transport, False)
        check_seal(pipe, (ks, hp), sp, sealed, perm, kind, transport, True)
        check_open(pipe, (ks, hp), sp, sealed, good(sp), perm, kind, transport)
    finally:
        pipe.close()
        ks.close()
        hp.close()


@pytest.mark.parametrize("transport,kind", [(COPY, "pageable"), (MAPPED, "pinned")], ids=["copy", "mapped"])
def test_rfc9001_a5_packet(engine, transport, kind):
    """the ChaCha20-Poly1305 short-header packet of RFC 9001 A.5 through quic_seal / quic_open, to the RFC's exact bytes (its
    sample is its whole tag and ends with the packet: pkt_len == pn_offset + 20)"""
    key = bytes.fromhex("c6d98ff3441c3fe1b2182094f69caa2ed4b716b65488960a7a984979fb23e1c8")
    iv = bytes.fromhex("e0459b3474bdd0e44a41c144")
    hpk = bytes.fromhex("25a282b9e82f06f21f488917a4fc8f1b73573685608597d0efcb076b0ab7a7a4")
    header, payload, pn = bytes.fromhex("4200bff4"), bytes.fromhex("01"), 654360564
    packet = bytes.fromhex("4cfe4189655e5cd55c41f69080575d7999c25a5bfb")
    ks = ptls_hip.KeySet(engine, 32, 3, algo=ptls_hip.ALGO_CHACHA20POLY1305)
    hp = ptls_hip.KeySet(engine, 32, 2, algo=ptls_hip.ALGO_CHACHA20POLY1305)
    ks.set(2, key, iv)
    hp.set(1, hpk, None)
    sp = [Spec(2, 1, header, 1, pn, pn - 1, payload)]
    pipe = pipeline(engine, "chacha", transport)
    try:
        check_seal(pipe, (ks, hp), sp, [packet], np.arange(1), kind, transport, False)
        check_open(pipe, (ks, hp), sp, [packet], good(sp), np.arange(1), kind, transport)
    finally:
        pipe.close()
        ks.close()
        hp.close()


def test_refusals(engine, keysets):
    """every refusal returns PTLS_HIP_EINVAL with its message (and the packet's index where one is at fault), every caller
    buffer stays at its prefill, the same objects then pass a correct call, and n == 0 succeeds"""
    L = ptls_hip.lib()
    sp = specs("runs")[::16]
    n = len(sp)
    sealed = protected("aes128", sp)
    pkt_offs, pkt_total = place([s.pkt_len for s in sp])
    data_offs, data_total = place([area(s) for s in sp])
    data_total += SLICE + 64  # room for the plaintext area of a packet too long for a slice (refused below)
    good_seal, good_open = descriptors(sp, pkt_offs, data_offs, False), descriptors(sp, pkt_offs, data_offs, True)
    ks, hp = keysets("aes128")
    ks256, hp256 = keysets("aes256")
    ksc, hpc = keysets("chacha")
    small = ptls_hip.KeySet(engine, 16, 4)
    engine2 = ptls_hip.Engine(engine.device)
    other = ptls_hip.KeySet(engine2, 16, NKEYS)
    pipe = pipeline(engine, "aes128", AUTO)
    pipec = pipeline(engine, "chacha", AUTO)
    # one host allocation for the packets and the plaintext, so that "h_out overlaps h_pkt" can be asked for
    pkt_img = image(mask_prefill(pkt_total), pkt_offs, sealed)
    both = np.concatenate([mask_prefill(data_total), pkt_img])
    both0 = both.copy()
    h_data, h_pkt = both[:data_total], both[data_total:]
    h_res, h_pn = np.full(n, SENTINEL, np.uint64), np.full(n, SENTINEL, np.uint64)
    k = next(i for i in range(n) if sp[i].slot >= 4)  # the first packet at fault is named
    kh = next(i for i in range(n) if sp[i].hp_slot >= 4)
    NULL = object()

    def ptr(x):
        return None if x is NULL else x.ctypes.data

    def seal(p=pipe, a=ks, h=hp, d=good_seal, cnt=n, i=h_data, pk=h_pkt):
        return L.ptls_hip_pipeline_quic_seal(p and p.ptr, a and a.ptr, h and h.ptr, ptr(d), cnt, ptr(i), ptr(pk))

    def open_(p=pipe, a=ks, h=hp, d=good_open, cnt=n, pk=h_pkt, o=h_data, r=h_res, pn=h_pn):
        return L.ptls_hip_pipeline_quic_open(p and p.ptr, a and a.ptr, h and h.ptr, ptr(d), cnt, ptr(pk), ptr(o), ptr(r), ptr(pn))

    def bad(base, field, value):
        d = base.copy()
        d[field][n - 2] = d["pn_offset"][n - 2] + 19 if value is None else value
        return d

    at = "packet %d:" % (n - 2)
    calls = [
        (lambda: seal(d=bad(good_seal, "pn_offset", 0)), [at, "pn_offset is 0"]),
        (lambda: open_(d=bad(good_open, "pn_offset", 0)), [at, "pn_offset is 0"]),
        (lambda: seal(d=bad(good_seal, "pkt_len", None)), [at, "pkt_len < pn_offset + 20"]),
        (lambda: open_(d=bad(good_open, "pkt_len", None)), [at, "pkt_len < pn_offset + 20"]),
        (lambda: seal(d=bad(good_seal, "pn_len", 0)), [at, "pn_len must be 1..4"]),
        (lambda: seal(d=bad(good_seal, "pn_len", 5)), [at, "pn_len must be 1..4"]),
        (lambda: seal(d=bad(good_seal, "pn", 1 << 62)), [at, "below 2^62"]),
        (lambda: seal(a=small), ["packet %d names key slot" % k]),
        (lambda: open_(a=small), ["packet %d names key slot" % k]),
        (lambda: seal(h=small), ["packet %d names header-protection key slot" % kh]),
        (lambda: open_(h=small), ["packet %d names header-protection key slot" % kh]),
        (lambda: seal(a=other), ["same engine"]),
        (lambda: open_(h=other), ["same engine"]),
        (lambda: seal(h=hp256), ["algorithm and key size"]),
        (lambda: open_(h=hp256), ["algorithm and key size"]),
        (lambda: seal(a=ks256), ["algorithm and key size"]),
        (lambda: seal(h=hpc), ["algorithm and key size"]),
        (lambda: open_(a=ksc), ["algorithm and key size"]),
        (lambda: seal(a=ksc, h=hpc), ["this pipeline serves AES-GCM keysets"]),
        (lambda: open_(p=pipec), ["this pipeline serves ChaCha20-Poly1305 keysets"]),
        (lambda: seal(p=None), ["null pipeline or keyset"]),
        (lambda: seal(a=None), ["null pipeline or keyset"]),
        (lambda: open_(h=None), ["null pipeline or keyset"]),
        (lambda: seal(d=NULL), ["null buffer"]),
        (lambda: seal(i=NULL), ["null buffer"]),
        (lambda: seal(pk=NULL), ["null buffer"]),
        (lambda: open_(d=NULL), ["null buffer"]),
        (lambda: open_(pk=NULL), ["null buffer"]),
        (lambda: open_(o=NULL), ["null buffer"]),
        (lambda: open_(r=NULL), ["null buffer"]),
        (lambda: open_(pn=NULL), ["null buffer"]),
        # the last plaintext area would end inside the first packet / the first area would start inside the last packet
        (lambda: open_(o=both[data_total + pkt_offs[0] + 1 - data_offs[-1] - area(sp[-1]):]), ["h_out overlaps the packets"]),
        (lambda: open_(o=both[data_total + pkt_offs[-1] + sp[-1].pkt_len - 1 - data_offs[0]:]), ["h_out overlaps the packets"]),
    ]
    for call, msgs in calls:
        assert call() == ptls_hip.EINVAL, msgs
        assert all(m in ptls_hip.last_error() for m in msgs), (msgs, ptls_hip.last_error())
    # MAPPED forced with pageable buffers; on COPY a packet that does not fit a slice
    pipe.set_transport(MAPPED)
    assert seal() == ptls_hip.EINVAL and "transport MAPPED needs" in ptls_hip.last_error(), ptls_hip.last_error()
    assert open_() == ptls_hip.EINVAL and "transport MAPPED needs" in ptls_hip.last_error(), ptls_hip.last_error()
    pipe.set_transport(AUTO)
    big = good_seal.copy()
    big["pkt_len"][1] = SLICE + 1
    assert seal(d=big) == ptls_hip.EINVAL
    assert "packet 1 does not fit a 65536-byte slice" in ptls_hip.last_error(), ptls_hip.last_error()
    big = good_open.copy()
    big["pkt_len"][2] = SLICE + 1
    assert open_(d=big) == ptls_hip.EINVAL
    assert "packet 2 does not fit a 65536-byte slice" in ptls_hip.last_error(), ptls_hip.last_error()
    # a buffer registered only in part: refused on every transport
    page = 4096
    raw = np.zeros(pkt_total + 3 * page, np.uint8)
    off = (-raw.ctypes.data) % page
    part = raw[off: off + pkt_total + page]
    part[:pkt_total] = pkt_img
    part0 = part.copy()
    assert pkt_total > page + 64 and L.ptls_hip_host_register(part.ctypes.data, page) == 0, ptls_hip.last_error()
    try:
        for tr in (MAPPED, AUTO, COPY):
            pipe.set_transport(tr)
            assert open_(pk=part) == ptls_hip.EINVAL and "registered only in part" in ptls_hip.last_error(), ptls_hip.last_error()
            assert seal(pk=part) == ptls_hip.EINVAL and "registered only in part" in ptls_hip.last_error(), ptls_hip.last_error()
    finally:
        L.ptls_hip_host_unregister(part.ctypes.data)
        pipe.set_transport(AUTO)
    # nothing was touched
    _same(both, both0, "a refused call wrote a caller buffer")
    _same(part, part0, "a refused call wrote a caller buffer")
    assert ints(h_res) == [SENTINEL] * n and ints(h_pn) == [SENTINEL] * n
    # n == 0 succeeds, whatever the buffers
    assert seal(d=NULL, cnt=0, i=NULL, pk=NULL) == 0 and open_(d=NULL, cnt=0, pk=NULL, o=NULL, r=NULL, pn=NULL) == 0
    _same(both, both0, "n == 0 wrote a caller buffer")
    # the same objects, used as they are meant to be
    assert open_() == 0, ptls_hip.last_error()
    assert pipe.last_transport == COPY
    _same(h_pkt, image(mask_prefill(pkt_total), pkt_offs, [s.header + x[len(s.header):] for s, x in zip(sp, sealed)]), "open h_pkt")
    _same(h_data, image(mask_prefill(data_total), data_offs, [s.payload for s in sp]), "open h_out")
    assert ints(h_res) == [len(s.payload) for s in sp] and ints(h_pn) == [s.pn for s in sp]
    h_in = image(mask_prefill(data_total), data_offs, [s.payload for s in sp])
    h_pkt[:] = image(mask_prefill(pkt_total), pkt_offs, [s.header for s in sp])
    assert seal(i=h_in) == 0, ptls_hip.last_error()
    _same(h_pkt, pkt_img, "seal h_pkt")
    for obj in (pipe, pipec, small, other, engine2):
        obj.close()
