"""The send object's cases (include/ptls_hip.h 2l), shared by tests/test_quic_tx_ref.py (hand-written statements about the
model), tests/test_quic_tx_native.py (the host build of hsig-picotls_amd/csrc/quic_tx.h) and tests/test_gpu_quic_tx.py (the
kernels).  A Call is a state table, a request list and the call's limits; want() is the model's outcome."""
import hashlib

import quic_tx_ref as model
from quic_tx_ref import Conn, NONE_ACKED, U64

NCONN = 130
STRIDE = 132     # the bank stride: above NCONN, so that the state count is what bounds a connection
HP_SLOTS = 131
PAYLOAD = 20


def cid(c, n=8):
    return hashlib.sha256(b"quic-tx-cid/%d" % c).digest()[:n]


class Call:
    def __init__(self, conns, reqs, in_len, buf_len, count=None, stride=STRIDE, hp_slots=HP_SLOTS, pn_len=0, rx_gens=None):
        self.conns, self.reqs, self.in_len, self.buf_len = conns, reqs, in_len, buf_len
        self.count = len(conns) if count is None else count
        self.stride, self.hp_slots, self.pn_len, self.rx_gens = stride, hp_slots, pn_len, rx_gens

    def want(self, conns=None):
        return model.seal(self.conns if conns is None else conns, self.reqs, self.count, self.stride, self.hp_slots, self.in_len,
                          self.buf_len, self.pn_len, self.rx_gens)

    def with_(self, **kw):
        c = Call(self.conns, self.reqs, self.in_len, self.buf_len, self.count, self.stride, self.hp_slots, self.pn_len, self.rx_gens)
        for k, v in kw.items():
            setattr(c, k, v)
        return c


def lay_out(items, tail=64):
    """items: (conn, len) -> requests with payloads back to back from offset 3 and packets at odd offsets with small gaps, each
    in an area of the largest size its packet can have; returns (reqs, in_len, buf_len)"""
    reqs, data, pkt = [], 3, 0
    for i, (conn, length) in enumerate(items):
        pkt += 1 + (i * 7) % 16
        if pkt % 2 == 0:
            pkt += 1
        reqs.append((data, pkt, conn, length))
        room = length if length <= 65535 else 0  # (a length no packet can hold takes no room: it is refused)
        data += room
        pkt += 1 + 20 + 4 + room + 16
    return reqs, data + 5, pkt + tail


# ---- the states of the case list: (name, Conn keyword arguments, payload lengths of the connection's run) ----

def _states():
    s = []
    add = lambda name, run=(PAYLOAD,), **kw: s.append((name, kw, run))  # noqa: E731
    add("a2-first", next_pn=0xac5c02, largest_acked=0xabe8b3)   # RFC 9000 A.2: 16 bits
    add("a2-second", next_pn=0xace8fe, largest_acked=0xabe8b3)  # ... 24 bits
    for k in (7, 15, 23, 31):  # num_unacked at 2^k - 1 and 2^k: the second request of the run crosses
        add("unacked-2^%d" % k, run=(PAYLOAD, PAYLOAD, PAYLOAD), next_pn=1000 + (1 << k) - 1, largest_acked=1000)
        add("unacked-2^%d-none" % k, run=(PAYLOAD, PAYLOAD), next_pn=(1 << k) - 2)  # no ack yet: num_unacked = pn + 1
    add("fresh", run=(PAYLOAD, PAYLOAD))
    add("pn-end", run=(PAYLOAD, PAYLOAD, PAYLOAD), next_pn=(1 << 62) - 1, largest_acked=(1 << 62) - 2)
    add("pn-saturates", run=(PAYLOAD, PAYLOAD, PAYLOAD), next_pn=U64 - 1, largest_acked=5)
    add("acked-equal", next_pn=500, largest_acked=500)
    add("acked-above", run=(PAYLOAD, PAYLOAD), next_pn=400, largest_acked=401)
    for n in (0, 8, 20):
        add("dcid-%d" % n, dcid_len=n)
    add("dcid-21", run=(PAYLOAD, PAYLOAD), dcid_len=21, next_pn=77, largest_acked=70)
    add("dcid-21-and-acked", dcid_len=21, next_pn=9, largest_acked=9)  # PN comes before RANGE
    for g in range(4):
        add("gen-%d" % g, gen=g, flags=g >> 1 & 1 ^ 1, next_pn=300 + g, largest_acked=299)
    add("gen-max", gen=0xFFFFFFFE, flags=1, next_pn=9000, largest_acked=100)
    add("short", run=(2, 3, 1, 0, 4, PAYLOAD), next_pn=50, largest_acked=49)  # one-byte numbers: 2, 1 and 0 bytes are too few
    add("short-2", run=(2, 1, 0), next_pn=50 + 128, largest_acked=49)         # two-byte numbers: 2 fits, 1 and 0 do not
    add("lengths", run=(3, 15, 16, 17, 63, 64, 65, 1350), next_pn=10, largest_acked=9)
    add("longest", run=(65535 - 1 - 8 - 1 - 16, 65535 - 1 - 8 - 1 - 16 + 1, PAYLOAD), next_pn=20, largest_acked=19)
    add("longest-no-dcid", run=(65535 - 1 - 2 - 16, 65535 - 1 - 2 - 16 + 1), dcid_len=0, next_pn=0x200, largest_acked=0x100)
    add("huge-len", run=(0xFFFFFFFF, 0xFFFFFFF0, PAYLOAD), next_pn=7, largest_acked=6)
    return s


STATES = _states()


def make_conns(count=NCONN):
    conns = []
    for c in range(count):
        _, kw, _ = STATES[c % len(STATES)]
        kw = dict(kw)
        n = kw.pop("dcid_len", 8)
        conns.append(Conn(dcid=cid(c, min(n, 20)), dcid_len=n, **kw))
    return conns


def case_list(pn_len=0, rx=None):
    """every state over 130 connections, in a connection order that is not ascending; behind them the requests no state
    explains: connections outside the table, second runs, offsets outside the buffers.  rx: None, or 'mixed' for receive-side
    generations below, at and above the send side's"""
    conns = make_conns()
    order = [(c * 37) % NCONN for c in range(NCONN)]
    items = []
    for k, c in enumerate(order):
        if k == 60:
            # connections outside: the count (130), the header-protection keyset (131), the stride (132), and the largest value
            items += [(NCONN, PAYLOAD), (NCONN + 1, PAYLOAD), (NCONN + 1, 2), (NCONN + 2, PAYLOAD), (0xFFFFFFFF, PAYLOAD),
                      (0xFFFFFFFF, 0xFFFFFFFF)]
            # second and third runs: A B A, of connections that send, of one that is refused (SPLIT comes before PN and RANGE)
            a, b, refused = order[0], order[1], next(x for x in order[:60] if STATES[x % len(STATES)][0] == "acked-equal")
            items += [(a, PAYLOAD), (a, PAYLOAD), (b, PAYLOAD), (a, 2), (refused, PAYLOAD), (b, PAYLOAD), (NCONN, PAYLOAD), (a, PAYLOAD)]
        items += [(c, length) for length in STATES[c % len(STATES)][2]]
    reqs, in_len, buf_len = lay_out(items)
    # the last packet ends with the buffer's last byte, the last payload with the input's: both ends pulled in
    last = model.seal(conns, reqs, NCONN, STRIDE, HP_SLOTS, in_len, buf_len, pn_len)
    assert last.status[-1] == model.SENT
    in_len, buf_len = reqs[-1][0] + reqs[-1][3], reqs[-1][1] + last.pkt_len[-1]
    # offsets outside the buffers by one byte, by a wrap, and at the ends, each behind the run of a connection that sends
    spare = [c for c in range(NCONN) if STATES[c % len(STATES)][0] == "fresh"]
    extra = [(data_off, pkt_off, spare[1 + k % 3], PAYLOAD)
             for k, (data_off, pkt_off) in enumerate([(in_len - PAYLOAD + 1, 1), (U64 - 3, 1), (U64, 1), (3, buf_len), (3, U64 - 40),
                                                      (3, U64), (in_len + 1, 1), (3, buf_len - 30)])]
    call_reqs = _merge(reqs, extra)
    assert call_reqs[-1] == reqs[-1]
    rx_gens = None
    if rx == "mixed":
        rx_gens = [max(0, conns[c].gen - 1) if c % 3 == 0 else conns[c].gen if c % 3 == 1 else min(conns[c].gen + 1 + c % 2, 0xFFFFFFFE)
                   for c in range(NCONN)]
    return Call(conns, call_reqs, in_len, buf_len, pn_len=pn_len, rx_gens=rx_gens)


def _merge(reqs, extra):
    """each extra request goes right behind the last request of its connection's FIRST run"""
    out = list(reqs)
    for e in extra:
        first = next(j for j, r in enumerate(out) if r[2] == e[2])
        end = first
        while end + 1 < len(out) and out[end + 1][2] == e[2]:
            end += 1
        out.insert(end + 1, e)
    return out


# ---- sizes: the passes' workgroups (256 threads) and the scan span (2 048) ----

def plain_conns(count, next_base=1000):
    return [Conn(next_pn=next_base + 3 * c, largest_acked=next_base + 3 * c - 1 - c % 200, gen=c % 3, dcid=cid(c), flags=c & 1)
            for c in range(count)]


def runs_call(lengths, count=NCONN, payload=PAYLOAD, **kw):
    """run r of lengths[r] requests on connection (r * 37) % count; len(lengths) <= count keeps every run numbered"""
    items = []
    for r, n in enumerate(lengths):
        items += [((r * 37) % count, payload)] * n
    reqs, in_len, buf_len = lay_out(items)
    return Call(plain_conns(count), reqs, in_len, buf_len, **kw)


def sized_call(n):
    """n requests in min(n, 100) runs of nearly equal length"""
    k = min(n, 100)
    return runs_call([n // k + (1 if r < n % k else 0) for r in range(k)])


def one_run_call(n=4096):
    return runs_call([n])


def edges_call():
    """runs that begin and end on workgroup edges, one request before and one behind them"""
    return runs_call([256, 1, 255, 512, 257, 255, 1, 1, 510])


def many_runs_call(k):
    """k runs of one request each on k connections (and one more run of two requests in front): the run indices cross the scan
    span at k = 2 048"""
    count = 2056
    return runs_call([1] * k, count=count, stride=count, hp_slots=count)


def lengths_call():
    """payload lengths 3, 15, 16, 17 and 1 350 on several connections, and the longest packet"""
    items = []
    for c, length in enumerate([3, 15, 16, 17, 1350, 3, 1350, 17, 16, 15]):
        items += [(c, length)] * (1 + c % 3)
    items += [(11, 65535 - 1 - 8 - 1 - 16), (12, PAYLOAD)]
    reqs, in_len, buf_len = lay_out(items)
    conns = [Conn(next_pn=5 + c, largest_acked=4 + c, gen=c % 3, dcid=cid(c)) for c in range(NCONN)]
    return Call(conns, reqs, in_len, buf_len)
