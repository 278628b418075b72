"""The datagram generator of the parse tests (tests/test_quic_parse_native.py on the CPU, tests/test_gpu_quic_parse.py on the
device): builders of QUIC packets with every field's encoding under the caller's control, and cases(), the families the
tests walk.  A case is (datagram bytes, bait bytes): the bait is what a truncation cut off, or bytes that would complete the
datagram's last field; the device test lays it right behind the datagram, where only an over-read can see it."""
import random

import quic_parse_ref as ref

# the connection IDs the generated packets mostly carry: the device test puts those of up to 20 bytes into its map
CID_POOL = [b"", b"\x07", bytes(range(8)), bytes(range(100, 120)), bytes([0x83, 0x94, 0xC8, 0xF0, 0x3E, 0x51, 0x57, 0x08]),
            bytes(8), bytes([0xFF] * 20), bytes(range(50, 58)), bytes(range(200, 204))]
TYPE_BITS = {ref.V1: {ref.INITIAL: 0, ref.ZERO_RTT: 1, ref.HANDSHAKE: 2, ref.RETRY: 3},
             ref.V2: {ref.RETRY: 0, ref.INITIAL: 1, ref.ZERO_RTT: 2, ref.HANDSHAKE: 3}}
UNKNOWN = 0x5A6A7A8A


def varint(v, width=None):
    """v as a varint of `width` bytes (1, 2, 4, 8; default: the shortest)"""
    if width is None:
        width = 1 if v < 64 else 2 if v < 16384 else 4 if v < 1 << 30 else 8
    assert v < 1 << (8 * width - 2)
    return (v | {1: 0, 2: 1, 4: 2, 8: 3}[width] << (8 * width - 2)).to_bytes(width, "big")


def long_packet(rng, version, typ, dcid, scid, token=b"", body_len=40, length=None, len_width=None, tok_width=None, fixed=True,
                bits=None):
    """a long-header packet; `length` overrides the Length field's value (default: body_len, what follows it).  Returns
    (bytes, pn_offset or 0).  For version 0 / UNKNOWN, `bits` chooses the type bits and the body is opaque."""
    if bits is None:
        bits = TYPE_BITS[version][typ] if version in TYPE_BITS else rng.randrange(4)
    first = 0x80 | (0x40 if fixed else 0) | bits << 4 | rng.randrange(16)
    h = bytes([first]) + version.to_bytes(4, "big") + bytes([len(dcid)]) + dcid + bytes([len(scid)]) + scid
    if version not in TYPE_BITS or typ == ref.RETRY:
        return h + rng.randbytes(body_len), 0
    if typ == ref.INITIAL:
        h += varint(len(token), tok_width) + token
    h += varint(body_len if length is None else length, len_width)
    return h + rng.randbytes(body_len), len(h)


def short_packet(rng, dcid, body_len=30, fixed=True):
    return bytes([(0x40 if fixed else 0) | rng.randrange(64)]) + dcid + rng.randbytes(body_len)


def _cid(rng, n=None):
    if n is None:
        return rng.choice(CID_POOL)
    pool = [c for c in CID_POOL if len(c) == n]
    return rng.choice(pool) if pool and rng.random() < 0.7 else rng.randbytes(n)


def _coalesced(rng, count, short_cid_len):
    """`count` packets in one datagram: long ones, the last one short half of the time"""
    d = b""
    for k in range(count):
        if k == count - 1 and rng.random() < 0.5:
            d += short_packet(rng, _cid(rng, short_cid_len), rng.randrange(20, 60))
        else:
            typ = rng.choice((ref.INITIAL, ref.ZERO_RTT, ref.HANDSHAKE))
            d += long_packet(rng, rng.choice((ref.V1, ref.V2)), typ, _cid(rng), _cid(rng), token=rng.randbytes(rng.choice((0, 0, 5))),
                             body_len=rng.randrange(20, 50), len_width=rng.choice((None, 1, 2, 4, 8)))[0]
    return d


def cases(seed=9000, random_fill=0):
    """yields (datagram, bait): the families of tests/test_quic_parse_native.py's docstring, then `random_fill` random ones"""
    rng = random.Random(seed)
    types = (ref.INITIAL, ref.ZERO_RTT, ref.HANDSHAKE, ref.RETRY)
    # every type under both versions, CID lengths 0 / 1 / 8 / 20, Length in every width (non-minimal ones included)
    for version in (ref.V1, ref.V2):
        for typ in types:
            for dl in (0, 1, 8, 20):
                for sl in (0, 1, 8, 20):
                    for width in (1, 2, 4, 8):
                        body = rng.choice((20, 21, 63)) if width == 1 else rng.choice((20, 63, 64, 300))
                        yield long_packet(rng, version, typ, _cid(rng, dl), _cid(rng, sl), token=rng.randbytes(rng.randrange(3)),
                                          body_len=body, len_width=width)[0], b""
    # version 0 and an unknown version, CID lengths up to 255; 21 under the known versions
    for version in (0, UNKNOWN, 0xFFFFFFFF, 2):
        for dl in (0, 1, 8, 20, 21, 255):
            for sl in (0, 8, 21, 255):
                yield long_packet(rng, version, None, rng.randbytes(dl) if dl > 20 else _cid(rng, dl), rng.randbytes(sl),
                                  body_len=rng.randrange(0, 40), fixed=rng.random() < 0.5)[0], b""
    for version in (ref.V1, ref.V2):
        for typ in types:
            for dl, sl in ((21, 0), (0, 21), (255, 8), (8, 255), (21, 21)):
                yield long_packet(rng, version, typ, rng.randbytes(dl), rng.randbytes(sl))[0], b""
    # token lengths at the varint boundaries, in the shortest and in wider encodings
    for version in (ref.V1, ref.V2):
        for tl in (0, 1, 63, 64, 16383, 16384):
            for tw in (None, 2 if tl < 16384 else 4, 8):
                yield long_packet(rng, version, ref.INITIAL, _cid(rng), _cid(rng), token=rng.randbytes(tl), tok_width=tw,
                                  body_len=rng.randrange(20, 40))[0], b""
    # coalesced runs of 1 .. 17 packets (the tests walk every case under max_per_dgram 1, 3 and 16)
    for count in range(1, 18):
        for scl in (0, 8, 20):
            yield _coalesced(rng, count, scl), b""
    # every truncation point of a long header: the datagram cut after each byte of the header in turn, and a little beyond
    for version in (ref.V1, ref.V2, 0, UNKNOWN):
        for typ in types:
            for tok, width in ((b"", 1), (rng.randbytes(70), 2), (rng.randbytes(3), 8)):
                pkt, pn_off = long_packet(rng, version, typ, _cid(rng, 8), _cid(rng, rng.choice((0, 8))), token=tok, body_len=24,
                                          len_width=width)
                lead = _coalesced(rng, 1, 8) if rng.random() < 0.3 else b""  # sometimes behind another packet
                for cut in range(1, (pn_off or len(pkt) - 24) + 22):
                    yield lead + pkt[:cut], pkt[cut:]
    # Length one below / one above what the datagram holds, Length 19 and 20, with bytes that would make it fit as the bait
    for version in (ref.V1, ref.V2):
        for typ in (ref.INITIAL, ref.ZERO_RTT, ref.HANDSHAKE):
            for width in (1, 2, 4, 8):
                for body, length in ((40, 39), (40, 41), (40, 40), (19, 19), (20, 20), (30, 19), (20, 21), (25, 1 << 14)):
                    if length >= 1 << (8 * width - 2):
                        continue
                    pkt = long_packet(rng, version, typ, _cid(rng), _cid(rng), body_len=body, length=length, len_width=width)[0]
                    yield pkt, rng.randbytes(max(1, length - body))
    # the fixed bit clear (the tests walk every case with the flag on and off)
    for version in (ref.V1, ref.V2, 0, UNKNOWN):
        for typ in types:
            yield long_packet(rng, version, typ, _cid(rng), _cid(rng), fixed=False)[0], b""
            yield _coalesced(rng, 2, 8) + long_packet(rng, version, typ, _cid(rng), _cid(rng), fixed=False)[0], b""
    for scl in (0, 8, 20):
        yield short_packet(rng, _cid(rng, scl), fixed=False), b""
    # short headers around the pn_offset + 20 limit for short_cid_len 0 / 8 / 20
    for scl in (0, 8, 20):
        for total in (1, 2, 20, 21, 22, scl + 20, scl + 21, scl + 22, 1350):
            pkt = short_packet(rng, _cid(rng, scl), 64)
            pkt = pkt + rng.randbytes(max(0, total - len(pkt)))
            yield pkt[:total], pkt[total:] + rng.randbytes(24)
    yield b"", b""
    for _ in range(random_fill):
        r = rng.random()
        if r < 0.5:
            d = _coalesced(rng, rng.randrange(1, 6), rng.choice((0, 8, 20)))
            cut = rng.randrange(len(d) + 1) if rng.random() < 0.5 else len(d)
            yield d[:cut], d[cut:]
        elif r < 0.8:  # a valid header with random damage
            d = bytearray(_coalesced(rng, rng.randrange(1, 4), 8))
            for _ in range(rng.randrange(1, 4)):
                d[rng.randrange(min(len(d), 40))] = rng.randrange(256)
            yield bytes(d), rng.randbytes(8)
        else:
            yield rng.randbytes(rng.randrange(1, 80)), rng.randbytes(8)
