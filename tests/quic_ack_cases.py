"""The cases of the ACK-frame call (include/ptls_hip.h 2m), shared by tests/test_quic_ack_native.py (the host build of
hsig-picotls_amd/csrc/quic_ack.h) and tests/test_gpu_quic_ack.py (the kernels), and an RFC 9000 §19.3 decoder that knows
nothing of windows: it reads a frame as a peer would and returns the packet numbers it acknowledges."""
import random

import quic_ack_ref as model

U64 = (1 << 64) - 1
COUNT = 130
ALTERNATING = 0x5555555555555555  # bits 0, 2, .. 62: 32 runs of one
# largest acknowledged = next - 1 at every varint edge, the window's own edges, the ends of the legal range and past it
NEXTS = [0, 1, 2, 3, 5, 63, 64, 65, 66, 100, 16384, 16385, (1 << 30), (1 << 30) + 1, (1 << 62) - 1, 1 << 62, (1 << 62) + 1, U64]
WINDOWS = [U64, 1, ALTERNATING, 1 | 1 << 63, 0b1011, 1 << 5, 0, U64 - 1, ALTERNATING << 1, 0x8000000000000001 | 0xFF << 20,
           0x00FF00FF00FF00FF, 0xF0F0F0F0F0F0F0F1, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFF00000001, 3 | 1 << 62]
DELAYS = [0, 63, 64, 16383, 16384, (1 << 30) - 1, 1 << 30, (1 << 62) - 1]
MAX_RANGES = [0, 1, 30, 31, 32, 0xFFFFFFFF]


# ---- the decoder ----

def read_varint(buf, at):
    """RFC 9000 §16 / A.1: (value, the position behind it)"""
    size = 1 << (buf[at] >> 6)
    value = buf[at] & 0x3F
    for b in buf[at + 1: at + size]:
        value = (value << 8) | b
    assert at + size <= len(buf)
    return value, at + size


def decode(buf, at=0):
    """the ACK frame at buf[at]: (largest acknowledged, ack delay, the acknowledged ranges as (highest, lowest) in frame order,
    the position behind the frame); RFC 9000 §19.3.1's arithmetic, which fails on a range that would go below 0"""
    assert buf[at] == 0x02
    largest, at = read_varint(buf, at + 1)
    delay, at = read_varint(buf, at)
    count, at = read_varint(buf, at)
    first, at = read_varint(buf, at)
    smallest = largest - first
    assert smallest >= 0
    ranges = [(largest, smallest)]
    for _ in range(count):
        gap, at = read_varint(buf, at)
        length, at = read_varint(buf, at)
        high = smallest - gap - 2
        smallest = high - length
        assert smallest >= 0
        ranges.append((high, smallest))
    return largest, delay, ranges, at


def acknowledged(ranges):
    return {pn for high, low in ranges for pn in range(low, high + 1)}


# ---- single entries ----

def grid():
    """(next, window): every edge of next against every window shape"""
    return [(n, w) for n in NEXTS for w in WINDOWS]


def stray_bits():
    """(next, window) for next in 1 .. 63: the window's legal bits and bits at k >= next, which count for nothing"""
    out = []
    for n in range(1, 64):
        legal = (ALTERNATING | 0b111) & ((1 << n) - 1)
        out += [(n, legal | 1 << n), (n, legal | (U64 << n) & U64), (n, legal | 1 << 63)]
    return out


def random_entries(k, seed):
    """k random windows with bit 0 set, of every density, against nexts around the window's reach and far from it"""
    rnd = random.Random(seed)
    out = []
    for _ in range(k):
        w = rnd.getrandbits(64)
        for _ in range(rnd.randrange(4)):
            w = w & rnd.getrandbits(64) if rnd.random() < 0.5 else w | rnd.getrandbits(64)
        n = rnd.choice([rnd.randrange(1, 130), rnd.randrange(1, 1 << 62), 1 << rnd.randrange(62)])
        out.append((n, w | 1))
    return out


# ---- whole calls ----

class Call:
    """a state table (3 * count entries of [next, window]), the space, the list, and the call's other parameters"""

    def __init__(self, count, spaces, space, conns, ack_delay=0, max_ranges=31, in_off=0, pkt_base=0, pkt_stride=0):
        assert len(spaces) == 3 * count
        self.count, self.spaces, self.space, self.conns = count, spaces, space, list(conns)
        self.ack_delay, self.max_ranges, self.in_off, self.pkt_base, self.pkt_stride = ack_delay, max_ranges, in_off, pkt_base, pkt_stride

    def with_(self, **kw):
        c = Call(self.count, self.spaces, self.space, self.conns, self.ack_delay, self.max_ranges, self.in_off, self.pkt_base, self.pkt_stride)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def permuted(self, seed):
        conns = list(self.conns)
        random.Random(seed).shuffle(conns)
        return self.with_(conns=conns)

    def want(self):
        return model.ack(self.spaces, self.count, self.space, self.conns, self.ack_delay, self.max_ranges, self.in_off, self.pkt_base,
                         self.pkt_stride)


def case_table(count=COUNT):
    """place p holds entry p of the grid, the stray-bit entries and 64 random ones, taken round: with 130 connections every
    space holds every shape somewhere, and the neighbours of an entry (the connection's other spaces) hold other entries"""
    entries = grid() + stray_bits() + random_entries(64, seed=11)
    step = 7  # (coprime to the number of entries: a space's places, 3 apart, walk through all of them)
    return [list(entries[(p * step) % len(entries)]) for p in range(3 * count)]


def case_list(space, count=COUNT, **kw):
    """every connection once in no ascending order, every eleventh twice, and connections outside the table"""
    conns = [(c * 37) % count for c in range(count)]
    conns += [c for c in range(0, count, 11)] + [count - 1, count, 0xFFFFFFFF, count + 5, count - 1]
    random.Random(space).shuffle(conns)
    return Call(count, case_table(count), space, conns, **kw)


def sized_call(n, count=40, seed=3, **kw):
    """n list entries over a small table: every twelfth connection is empty, every twelfth has no acceptable state, and about
    one entry in twenty lies outside the table"""
    rnd = random.Random(seed * 100003 + n)
    spaces = []
    for p in range(3 * count):
        kind = (p // 3) % 12
        nxt = rnd.choice([1, 7, 64, 65, 1000, 16384, 1 << 30, 1 << 40])
        spaces.append([0, 0] if kind == 0 else [nxt, rnd.getrandbits(64) & ~1] if kind == 1 else [nxt, rnd.getrandbits(64) | 1])
    conns = [rnd.randrange(count + 2) for _ in range(n)]
    return Call(count, spaces, 2, conns, **kw)


def empty_call(n=300, count=9):
    """every list entry ACK_EMPTY in the space asked for; the other spaces hold states that would give frames"""
    spaces = [[0, 0] if p % 3 == 1 else [50 + p, U64] for p in range(3 * count)]
    return Call(count, spaces, 1, [j % count for j in range(n)], pkt_stride=64)


def edge_call(ack_delay, n=520):
    """the shortest and the longest frame of a call next to each other, across the workgroup edges at 256 and 512: even
    positions one range and a 1-byte largest, odd ones 31 further ranges and an 8-byte largest.  The delay is the call's, so a
    frame of 5 bytes (1-byte delay) and one of 81 (8-byte delay) cannot meet in one call: with ack_delay 0 the lengths are 5 and
    74, with 2^62 - 1 they are 12 and 81"""
    spaces = [[1, 1]] * 3 + [[1 << 62, ALTERNATING]] * 3
    return Call(2, [list(s) for s in spaces], 0, [j % 2 for j in range(n)], ack_delay=ack_delay, pkt_base=5, pkt_stride=128)
