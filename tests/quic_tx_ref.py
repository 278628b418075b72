"""Plain-Python model of the send object (include/ptls_hip.h 2l): integers and bytes only.  What a send call gives every
request (status, packet number, packet length, header bytes, key slot) and the state table after it, from the state before
it; packet bytes go through quic_ref.protect.

A connection is a Conn (next_pn, largest_acked, gen, dcid, flags, dcid_len); dcid_len defaults to len(dcid) and may be set
above 20 to model a corrupt entry (the table still holds 20 bytes).  A request is (data_off, pkt_off, conn, len)."""
import quic_ref

U64 = (1 << 64) - 1
NONE_ACKED = U64
SENT, NO_CONN, SPLIT, PN, RANGE = range(5)
PN_END = 1 << 62


class Conn:
    def __init__(self, next_pn=0, largest_acked=NONE_ACKED, gen=0, dcid=b"", flags=0, dcid_len=None):
        assert len(dcid) <= 20
        self.next_pn, self.largest_acked, self.gen, self.dcid, self.flags = next_pn, largest_acked, gen, bytes(dcid), flags
        self.dcid_len = len(dcid) if dcid_len is None else dcid_len

    def copy(self):
        return Conn(self.next_pn, self.largest_acked, self.gen, self.dcid, self.flags, self.dcid_len)

    def key(self):
        return (self.next_pn, self.largest_acked, self.gen, self.dcid, self.flags, self.dcid_len)

    def __eq__(self, other):
        return self.key() == other.key()

    def __repr__(self):
        return "Conn%r" % (self.key(),)


def pn_len(pn, largest_acked, min_len=0):
    """RFC 9000 §17.1 / A.2: the smallest length in max(1, min_len) .. 4 whose range is more than twice num_unacked; 0: none"""
    num_unacked = pn + 1 if largest_acked == NONE_ACKED else pn - largest_acked
    for length in range(max(1, min_len), 5):
        if num_unacked < 1 << (8 * length - 1):
            return length
    return 0


def first_byte(flags, gen, length):
    return 0x40 | (flags & 1) << 5 | (gen & 1) << 2 | (length - 1)


def header(conn, gen, pn, length):
    return bytes([first_byte(conn.flags, gen, length)]) + conn.dcid[:conn.dcid_len] + (pn & ((1 << (8 * length)) - 1)).to_bytes(length, "big")


def judge(req, pn, conn, in_len, buf_len, min_len):
    """rules 4 to 6: (status, pn_len, pkt_len)"""
    data_off, pkt_off, _, length = req
    if pn >= PN_END or (conn.largest_acked != NONE_ACKED and conn.largest_acked >= pn):
        return PN, 0, 0
    L = pn_len(pn, conn.largest_acked, min_len)
    if L == 0:
        return PN, 0, 0
    if conn.dcid_len > 20 or L + length < 4:
        return RANGE, 0, 0
    pkt_len = 1 + conn.dcid_len + L + length + 16
    if pkt_len > 65535 or data_off + length > in_len or pkt_off + pkt_len > buf_len:
        return RANGE, 0, 0
    return SENT, L, pkt_len


class Outcome:
    """status / pn_out / pkt_len per request; for a sent request also headers[j], gens[j], slots[j] (else None); conns = the
    state table after the call"""

    def __init__(self, n):
        self.status, self.pn_out, self.pkt_len = [None] * n, [U64] * n, [0] * n
        self.headers, self.gens, self.slots = [None] * n, [None] * n, [None] * n
        self.conns = None

    @property
    def sent(self):
        return [j for j, s in enumerate(self.status) if s == SENT]


def seal(conns, reqs, count, stride, hp_slots, in_len, buf_len, min_len=0, rx_gens=None):
    """the whole rule; conns is not modified.  rx_gens: per connection below count, the receive side's generation, or None"""
    assert len(conns) >= count and (rx_gens is None or len(rx_gens) >= count)
    nconn = min(count, stride, hp_slots)
    out = Outcome(len(reqs))
    after = [c.copy() for c in conns]
    first = {}
    runs = []  # (head, length)
    for j, r in enumerate(reqs):
        if j == 0 or reqs[j - 1][2] != r[2]:
            runs.append([j, 0])
            if r[2] < nconn:
                first.setdefault(r[2], j)
        runs[-1][1] += 1
    for h, length in runs:
        c = reqs[h][2]
        for j in range(h, h + length):
            if c >= nconn:
                out.status[j] = NO_CONN
            elif first[c] != h:
                out.status[j] = SPLIT
            else:
                conn = conns[c]
                gen = conn.gen if rx_gens is None else max(conn.gen, rx_gens[c])
                pn = min(conn.next_pn + (j - h), U64)
                out.pn_out[j] = pn
                out.status[j], L, out.pkt_len[j] = judge(reqs[j], pn, conn, in_len, buf_len, min_len)
                if out.status[j] == SENT:
                    out.headers[j], out.gens[j], out.slots[j] = header(conn, gen, pn, L), gen, c + stride * (gen % 3)
        if c < nconn and first[c] == h:
            after[c].next_pn = min(conns[c].next_pn + length, U64)
            after[c].gen = conns[c].gen if rx_gens is None else max(conns[c].gen, rx_gens[c])
    out.conns = after
    return out


def packet(algo, key, iv, hp_key, hdr, pn, payload):
    """the protected packet of a sent request"""
    return quic_ref.protect(algo, key, iv, hp_key, hdr, pn, payload)
