"""Plain-Python reference of QUIC datagram parsing (include/ptls_hip.h 2h): the varint decode of RFC 9000 §16, the walk of one
packet, the entries of a datagram with max_per_dgram and MORE, the output records of ptls_hip_quic_parse_datagrams, and a
dict-backed connection-ID map.  This file is the normative statement of the ORDER of the parse rules;
hsig-picotls_amd/csrc/quic_parse.h restates it and is checked against it (tests/test_quic_parse_native.py on the CPU,
tests/test_gpu_quic_parse.py on the device).  Nothing here looks at a byte at or past the end of the datagram it is given:
every packet is walked on the slice `d` = [its first byte, the datagram's end)."""

(INITIAL, ZERO_RTT, HANDSHAKE, RETRY, ONE_RTT, VERSION_NEGOTIATION, UNKNOWN_VERSION, NONE) = range(8)
(OK, TRUNCATED, TOO_SHORT, BAD_CID_LEN, BAD_FIXED_BIT) = range(5)
MORE = 1
NO_CONN = 0xFFFFFFFF
V1, V2 = 0x00000001, 0x6B3343CF
MAX_CID = 20
MIN_PROTECTED = 20  # packet number, payload and tag behind pn_offset: the header-protection sample ends at pn_offset + 20
WALK_FIELDS = ("status", "type", "version", "dcid_off", "dcid_len", "scid_off", "scid_len", "token_off", "token_len", "pn_offset",
               "pkt_len")


def varint(d, pos):
    """(value, next position) of the varint at d[pos], or None when it does not fit into d"""
    if pos >= len(d):
        return None
    n = 1 << (d[pos] >> 6)
    if n > len(d) - pos:
        return None
    v = d[pos] & 0x3F
    for b in d[pos + 1: pos + n]:
        v = (v << 8) | b
    return v, pos + n


def walk_packet(d, short_cid_len, require_fixed_bit):
    """the packet at the start of d = the bytes from its first byte to the datagram's end (at least one)"""
    d = bytes(d)
    rest = len(d)
    w = dict.fromkeys(WALK_FIELDS, 0)
    w.update(status=TRUNCATED, type=NONE, pkt_len=rest)

    def end(status):
        w["status"] = status
        return w

    first = d[0]
    fixed_bad = bool(require_fixed_bit) and not first & 0x40
    if not first & 0x80:
        w["type"] = ONE_RTT
        if fixed_bad:
            return end(BAD_FIXED_BIT)
        if rest < 1 + short_cid_len + MIN_PROTECTED:
            return end(TOO_SHORT)
        w.update(dcid_off=1, dcid_len=short_cid_len, pn_offset=1 + short_cid_len)
        return end(OK)
    if rest < 5:
        return end(TRUNCATED)
    version = int.from_bytes(d[1:5], "big")
    known = version in (V1, V2)
    bits = (first >> 4) & 3
    w["version"] = version
    w["type"] = (VERSION_NEGOTIATION if version == 0 else (INITIAL, ZERO_RTT, HANDSHAKE, RETRY)[bits] if version == V1 else
                 (RETRY, INITIAL, ZERO_RTT, HANDSHAKE)[bits] if version == V2 else UNKNOWN_VERSION)
    if known and fixed_bad:
        return end(BAD_FIXED_BIT)
    if rest < 6:
        return end(TRUNCATED)
    dl = d[5]
    if known and dl > MAX_CID:
        return end(BAD_CID_LEN)
    if 6 + dl >= rest:  # the DCID and the SCID length behind it
        return end(TRUNCATED)
    w.update(dcid_off=6, dcid_len=dl)
    sl = d[6 + dl]
    if known and sl > MAX_CID:
        return end(BAD_CID_LEN)
    pos = 7 + dl + sl
    if pos > rest:
        return end(TRUNCATED)
    w.update(scid_off=7 + dl, scid_len=sl)
    if not known or w["type"] == RETRY:
        return end(OK)
    if w["type"] == INITIAL:
        t = varint(d, pos)
        if t is None or t[0] > rest - t[1]:
            return end(TRUNCATED)
        w.update(token_off=t[1], token_len=t[0])
        pos = t[1] + t[0]
    t = varint(d, pos)
    if t is None:
        return end(TRUNCATED)
    length, pos = t
    if length < MIN_PROTECTED:
        return end(TOO_SHORT)
    if length > rest - pos:
        return end(TRUNCATED)
    w.update(pn_offset=pos, pkt_len=pos + length)
    return end(OK)


def walk_datagram(d, short_cid_len, max_per_dgram, require_fixed_bit):
    """[(position, walk, more)] of the datagram d, in wire order"""
    d = bytes(d)
    out, pos = [], 0
    while pos < len(d) and len(out) < max_per_dgram:
        w = walk_packet(d[pos:], short_cid_len, require_fixed_bit)
        nxt = pos + w["pkt_len"]
        out.append((pos, w, len(out) + 1 == max_per_dgram and nxt < len(d)))
        pos = nxt
    return out


def pn_space(t):
    return 0 if t == INITIAL else 1 if t == HANDSHAKE else 2


class CidMap:
    """what ptls_hip_quic_cidmap_t does, over a dict"""

    def __init__(self, capacity):
        self.capacity, self.d = capacity, {}

    def set(self, cid, conn):
        cid = bytes(cid)
        if len(cid) > MAX_CID or conn == NO_CONN or (cid not in self.d and len(self.d) >= self.capacity):
            raise ValueError("refused")
        self.d[cid] = conn

    def remove(self, cid):
        self.d.pop(bytes(cid), None)

    def lookup(self, cid):
        return self.d.get(bytes(cid), NO_CONN) if len(cid) <= MAX_CID else NO_CONN

    def __len__(self):
        return len(self.d)


def cid_hash(cid):
    """the map's hash (csrc/quic_parse.h quic_cid_hash): FNV-1a over the length and every byte, then MurmurHash3's finalizer;
    an entry's home slot is this value's low bits.  Here so that a test can build probe chains where it wants them."""
    m = 0xFFFFFFFF
    h = ((2166136261 ^ len(cid)) * 16777619) & m
    for b in cid:
        h = ((h ^ b) * 16777619) & m
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & m
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & m
    h ^= h >> 16
    return h


def parse_datagrams(buf, dgrams, short_cid_len=0, max_per_dgram=16, require_fixed_bit=1, cidmap=None, expected_pn=None,
                    expected_count=None):
    """what ptls_hip_quic_parse_datagrams returns for the datagrams [(off, len)] in buf: a list of (packet dict, info dict),
    with the field names of ptls_hip_quic_packet_t and ptls_hip_quic_pktinfo_t.  cidmap: a CidMap or None; expected_pn: a
    sequence indexed 3 * conn + space, or None; expected_count: how many of its entries count (default: all)."""
    if expected_pn is not None and expected_count is None:
        expected_count = len(expected_pn)
    out = []
    for i, (off, ln) in enumerate(dgrams):
        d = bytes(buf[off: off + ln])
        for pos, w, more in walk_datagram(d, short_cid_len, max_per_dgram, require_fixed_bit):
            conn = NO_CONN
            if w["status"] == OK and cidmap is not None:
                p = d[pos:]
                conn = cidmap.lookup(p[w["dcid_off"]: w["dcid_off"] + w["dcid_len"]])
            pn = 0
            if w["pn_offset"] != 0 and expected_pn is not None and conn != NO_CONN:
                e = conn * 3 + pn_space(w["type"])
                if e < expected_count:
                    pn = int(expected_pn[e])
            pkt = dict(pkt_off=off + pos, data_off=off + pos + w["pn_offset"] + 1, pn=pn, pkt_len=w["pkt_len"], key=conn,
                       hp_key=conn, pn_offset=w["pn_offset"], pn_len=0, flags=0)
            info = dict(dgram=i, version=w["version"], conn=conn, token_len=w["token_len"], dcid_off=w["dcid_off"],
                        scid_off=w["scid_off"], token_off=w["token_off"], dcid_len=w["dcid_len"], scid_len=w["scid_len"],
                        type=w["type"], status=w["status"], flags=MORE if more else 0)
            out.append((pkt, info))
    return out


def to_arrays(entries):
    """the reference's entries as the numpy arrays the binding returns (QUIC_PACKET_DTYPE, QUIC_PKTINFO_DTYPE; pad = 0)"""
    import numpy as np
    import ptls_hip
    pkts = np.zeros(len(entries), dtype=ptls_hip.QUIC_PACKET_DTYPE)
    info = np.zeros(len(entries), dtype=ptls_hip.QUIC_PKTINFO_DTYPE)
    for k, (p, f) in enumerate(entries):
        for name, v in p.items():
            pkts[name][k] = v
        for name, v in f.items():
            info[name][k] = v
    return pkts, info
