"""The cases of the packet-number tracking tests (include/ptls_hip.h 2k), shared by the CPU checks (tests/test_quic_track_ref.py,
tests/test_quic_track_native.py) and the GPU tests (tests/test_gpu_quic_track.py).  Nothing here calls the library: what every
packet must get and every space must become is tests/quic_track_ref.py's.

A Call is one track call: the connection count, the state table before it, and the selected packets in selected order as
(connection, type, result, packet number)."""
import functools
import random

import quic_track_ref as model

U64 = model.U64
TOP = (1 << 62) - 1  # the largest packet number (RFC 9000 §12.3)
SHIFTS = (0, 1, 63, 64, 65, 1 << 40)
TYPES_OF_SPACE = {0: (model.INITIAL,), 1: (model.HANDSHAKE,), 2: (model.ONE_RTT, model.ZERO_RTT)}
UNTRACKED_TYPES = (model.RETRY, model.VERSION_NEGOTIATION, model.UNKNOWN_VERSION, model.NO_TYPE)
CLAIM_PER_THREAD, WG = 4, 256  # csrc/internal.h QTK_CLAIM_PER_THREAD; the kernels' workgroup


class Call:
    def __init__(self, count, spaces, packets, expected_len=None):
        assert len(spaces) == 3 * count
        self.count, self.spaces, self.packets = count, [list(s) for s in spaces], list(packets)
        self.expected_len = 3 * count if expected_len is None else expected_len

    def columns(self):
        return tuple(list(col) for col in zip(*self.packets)) if self.packets else ([], [], [], [])

    def want(self, expected=None, spaces=None):
        """the model's (verdicts, touched, spaces after, expected after) from `spaces` (default: the call's own) and an
        expected-pn table `expected` (a list, or None for no table)"""
        after = [list(s) for s in (self.spaces if spaces is None else spaces)]
        exp = list(expected) if expected is not None else None
        verdicts, touched = model.track(after, exp, self.count, *self.columns())
        return verdicts, touched, after, exp

    def permuted(self, seed):
        pk = list(self.packets)
        random.Random(seed).shuffle(pk)
        return Call(self.count, self.spaces, pk, self.expected_len)


def states():
    """(next, window) pairs that a receiver can be in: bit 0 is set wherever something was accepted, no bit below packet 0"""
    out = [(0, 0)]
    for next_ in (1, 2, 64, 65, 66, 1000, (1 << 40) + 5, TOP - 70, TOP + 1):
        reach = min(next_, 64)
        for pattern in (1, (1 << 64) - 1, 0x5555555555555555, 1 | 1 << 63, 1 | 1 << 62):
            window = pattern % (1 << reach) | 1
            if (next_, window) not in out:
                out.append((next_, window))
    return out


def candidates(next_, window):
    """packet numbers around every boundary of a state: next - 1 - pn of 0, 1, 62, 63, 64, 65; shifts of SHIFTS; 2^62 - 1"""
    out = [next_ - 1 - back for back in (0, 1, 2, 62, 63, 64, 65, 1000) if next_ - 1 - back >= 0]
    out += [next_ - 1 + shift for shift in SHIFTS[1:] + (2, 66) if 0 <= next_ - 1 + shift <= TOP]
    out.append(TOP)
    return sorted(set(out))


@functools.lru_cache(maxsize=None)
def grid():
    """one space at a time: (next, window, [(result, pn), ...]): every candidate alone, every ordered pair of candidates (both
    orders of every pair, a number with itself included), each pair again with its first packet failed, and every number three
    times over with another between the copies"""
    out = []
    for next_, window in states():
        cand = candidates(next_, window)
        for a in cand:
            out.append((next_, window, [(20, a)]))
            out.append((next_, window, [(20, a), (0, a), (1200, a)]))
            out.append((next_, window, [(20, a), (20, cand[0]), (20, a), (U64, a), (20, a)]))
            for b in cand:
                out.append((next_, window, [(20, a), (20, b)]))
                out.append((next_, window, [(U64, a), (20, b)]))
    return out


def single(case, count=3, conn=1, space=2, other=(77, 0b1011)):
    """a grid case as a Call of its own: the case in one space, every other space in a state that must not change"""
    next_, window, pk = case
    spaces = [list(other) for _ in range(3 * count)]
    spaces[3 * conn + space] = [next_, window]
    types = TYPES_OF_SPACE[space]
    return Call(count, spaces, [(conn, types[k % len(types)], result, pn) for k, (result, pn) in enumerate(pk)])


NCONN = 130


def case_list(part, parts=3, count=NCONN, seed=0):
    """Part `part` of `parts` of the grid laid over the 3 * count spaces of one call (as many grid cases as there are spaces,
    taken at an even stride so that every state and every boundary is met), shuffled, with between them: packets of the
    connections count - 1 (tracked) and count and above (not tracked), types without a packet-number space, a failed packet
    with the largest number of the call in a space of its own, and all three spaces of one connection with the same numbers"""
    g = grid()
    places = 3 * count
    rng = random.Random(1000 * parts + part + seed)
    picked = [g[(part + parts * k * (len(g) // (parts * places))) % len(g)] for k in range(places)]
    spaces, packets = [], []
    for place, (next_, window, pk) in enumerate(picked):
        conn, space = divmod(place, 3)
        spaces.append([next_, window])
        types = TYPES_OF_SPACE[space]
        packets += [(conn, types[(place + k) % len(types)], result, pn) for k, (result, pn) in enumerate(pk)]
    # connection 7: the same state and the same numbers in all three spaces, which stay apart
    for s in range(3):
        spaces[21 + s] = [500, 0b10011]
    packets = [p for p in packets if p[0] != 7]
    for pn in (499, 498, 497, 496, 495, 436, 435, 500, 502, 502):
        packets += [(7, TYPES_OF_SPACE[s][0], 20, pn) for s in range(3)]
    packets.append((7, model.HANDSHAKE, 20, 600))  # ... and one of them moves on alone
    # connection count - 1 is inside; count and count + 1 are outside
    packets += [(count - 1, model.ONE_RTT, 20, TOP - 1), (count, model.ONE_RTT, 20, 5), (count + 1, model.INITIAL, 20, 5)]
    # types without a space, and a failed packet with the largest number of the call
    packets += [(3, t, 20, 1 << 50) for t in UNTRACKED_TYPES]
    packets += [(c, model.ONE_RTT, U64, TOP) for c in (0, 5, count - 1)]
    rng.shuffle(packets)
    return Call(count, spaces, packets, expected_len=places - 5)  # (the last spaces lie outside the expected-pn table)


def claim_threads(m):
    return WG * -(-m // (WG * CLAIM_PER_THREAD))


BULK = 4096


@functools.lru_cache(maxsize=None)
def bulk_call():
    """4 096 packets in buffer order, almost all fresh 1-RTT packets of connection 0, laid out for the groupings of the claim
    pass.  Thread t of 1 024 takes packets t, t + 1 024, t + 2 048 and t + 3 072, so a wave of threads sees four rows:
      most waves  connection 0, space 2, ascending numbers: folded three times, then reduced to one atomic per wave; the
                  largest number of the call sits in row 1 at lane 37 of wave 1
      wave 4      space 2, then space 0 (Initial), then space 2 again: the space changes (flushes), the wave ends on one space
      wave 5      spaces 2 and 1 (Handshake) in alternating lanes: two spaces in one wave
      wave 6      lanes 10..20 failed in every row, with huge numbers: lanes that hold nothing beside lanes that do
      wave 7      space 2, but lane 27 ends in row 3 on connection 1: two places again
    Space 2 of connection 0 starts at (1000, all ones) and every packet of it is new: it ends with an all-ones window."""
    T = claim_threads(BULK)
    assert T == 1024
    spaces = [[0, 0], [40, 1], [1000, (1 << 64) - 1], [0, 0], [0, 0], [7, 0b1000001]]
    counter = {}
    packets = []

    def fresh(conn, type_, base):
        k = counter.get((conn, type_), 0)
        counter[(conn, type_)] = k + 1
        return (conn, type_, 20, base + k)

    for j in range(BULK):
        row, t = divmod(j, T)
        w, lane = divmod(t, 64)
        if w == 4 and row == 1:
            packets.append(fresh(0, model.INITIAL, 0))
        elif w == 5 and lane % 2 == 1:
            packets.append(fresh(0, model.HANDSHAKE, 100))
        elif w == 6 and 10 <= lane <= 20:
            packets.append((0, model.ONE_RTT, U64, TOP - j))
        elif w == 7 and row == 3 and lane == 27:
            packets.append(fresh(1, model.ONE_RTT, 7))
        else:
            packets.append(fresh(0, model.ONE_RTT, 1000))
    # the largest number of space 2 changes places with the one in row 1, lane 37 of wave 1
    ones = [j for j, p in enumerate(packets) if p[:2] == (0, model.ONE_RTT) and p[2] != U64]
    a, b = ones[-1], T + 64 + 37
    assert b in ones
    packets[a], packets[b] = packets[b], packets[a]
    return Call(2, spaces, packets)


def claim_paths(call):
    """which groupings the claim pass goes through for a call, from its geometry (thread t of T = claim_threads(m) takes
    packets t, t + T, ...; the device has more workgroups than that): counts of folds (a lane's successive candidates of one
    space), of flushes (the space changed), and of waves that end with one space held by several lanes ("reduce"), of those
    with lanes that hold nothing ("partial"), and with two spaces or more ("split"); the lanes that held a reduced wave's top"""
    m = len(call.packets)
    T = claim_threads(m)
    out = dict(fold=0, flush=0, reduce=0, partial=0, split=0, top_lanes=set())
    final = []
    for t in range(T):
        at, top = None, 0
        for j in range(t, m, T):
            conn, type_, result, pn = call.packets[j]
            if not model.tracked(conn, type_, result, call.count):
                continue
            place = 3 * conn + model.SPACE_OF[type_]
            next_, window = call.spaces[place]
            if pn < next_ and (next_ - 1 - pn >= model.WINDOW or pn in model.accepted(next_, window)):
                continue
            if place == at:
                out["fold"] += 1
                top = max(top, pn + 1)
            else:
                out["flush"] += at is not None
                at, top = place, pn + 1
        final.append((at, top))
    for w in range(0, T, 64):
        held = [(lane, at, top) for lane, (at, top) in enumerate(final[w: w + 64]) if at is not None]
        if len({at for _, at, _ in held}) > 1:
            out["split"] += 1
        elif len(held) > 1:
            out["reduce"] += 1
            out["partial"] += len(held) < 64
            out["top_lanes"].add(max(held, key=lambda h: h[2])[0])
    return out


def distinct_call(m, count=7):
    """m packets, every (space, number) once, over all spaces of `count` connections, from empty states: all new"""
    packets = [(j % count, (model.INITIAL, model.HANDSHAKE, model.ONE_RTT, model.ZERO_RTT)[(j // count) % 4], 20, 3 * j + j % 5)
               for j in range(m)]
    return Call(count, [[0, 0]] * (3 * count), packets)


def copies_call(m=257):
    """m copies of one packet: position 0 is new, the others duplicates of it"""
    return Call(2, [[0, 0]] * 3 + [[90, 1]] * 3, [(1, model.ONE_RTT, 20, 95)] * m)


def triples_call(m=2049, keys=300):
    """`keys` numbers three times each at positions k, k + keys and k + 2 keys, so that most triples have their copies in three
    workgroups of both packet passes; distinct packets of another space behind them"""
    packets = [(0, model.ONE_RTT, 20, 10 + 2 * (j % keys)) for j in range(3 * keys)]
    packets += [(0, model.HANDSHAKE, 20, j) for j in range(m - 3 * keys)]
    return Call(1, [[0, 0]] * 3, packets)


def spread_triples(call, keys=300):
    """the triples of triples_call whose three copies lie in three workgroups of the claim pass and of the verdict pass"""
    T = claim_threads(len(call.packets))
    return [k for k in range(keys)
            if len({(j % T) // WG for j in (k, k + keys, k + 2 * keys)}) == 3 and len({j // WG for j in (k, k + keys, k + 2 * keys)}) == 3]


def seam_call(count):
    """one packet per connection around one scan span of the touched list: every fifth connection and the last ones receive a
    new packet, every tenth of the rest a failed one, the others a duplicate of what their window holds"""
    spaces = [[10 + c % 3, 1] for c in range(count) for _ in range(3)]
    packets = []
    for c in range(count):
        top = spaces[3 * c + 2][0] - 1
        if c % 5 == 0 or c in (count - 1, 2046, 2047):
            packets.append((c, model.ONE_RTT, 20, top + 1 + c % 7))
        elif c % 10 == 3:
            packets.append((c, model.ONE_RTT, U64, top + 1 + c % 7))
        else:
            packets.append((c, model.ONE_RTT, 20, top))
    random.Random(count).shuffle(packets)
    return Call(count, spaces, packets)
