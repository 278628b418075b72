"""The cases of the key-phase tests (include/ptls_hip.h 2j), shared by the CPU check of the case list against the reference
(tests/test_quic_phase_ref.py) and the GPU tests (tests/test_gpu_quic_keyphase.py).  Nothing here calls the library: keys
come from tests/quic_keys_ref.py ("quic ku" steps from one secret per connection), packets from tests/quic_ref.py, and what
each packet must do from tests/quic_phase_ref.py.

A case is a Case: the per-connection states, the key material of every generation, and packets in the order they lie in the
buffer, each with the generation it was SEALED under (`sealed`; for a long header: the generation whose keys sit in the
connection's own slot) and the generation the rule must CHOOSE (`want_gen`); it must open if and only if the two agree."""
import functools
import hashlib
import random

import quic_keys_ref
import quic_phase_ref as model
import quic_ref

U64 = model.U64
NGENS = 8
PAYLOADS = (0, 1, 16, 17, 100, 1200)
# (pn_len, payload bytes) with the header-protection sample inside the packet
SHAPES = tuple((pn_len, L) for L in PAYLOADS for pn_len in (1, 2, 3, 4) if pn_len + L >= 4)
HASH_SIZE = 32


def stream(tag, n):
    out, i = bytearray(), 0
    while len(out) < n:
        out += hashlib.sha256(b"%s/%d" % (tag.encode(), i)).digest()
        i += 1
    return bytes(out[:n])


PAYLOAD = stream("quic-phase-payload", 4096)
CID = stream("quic-phase-cid", 4096)


@functools.lru_cache(maxsize=None)
def material(algo, nconn, ngens=NGENS):
    """(keys[c][g] = (key, iv) of generation g of connection c, hps[c] = its header-protection key, which no update changes)"""
    ksz = quic_ref.KEY_SIZE[algo]
    keys, hps = [], []
    for c in range(nconn):
        secret = stream("quic-phase-%s-secret-%d" % (algo, c), HASH_SIZE)
        hps.append(quic_keys_ref.keys(secret, ksz, check=False)[2])
        row = []
        for _ in range(ngens):
            key, iv, _hp = quic_keys_ref.keys(secret, ksz, check=False)
            row.append((key, iv))
            secret = quic_keys_ref.update(secret, check=False)
        keys.append(row)
    return keys, hps


class Packet:
    def __init__(self, conn, sealed, header, pn_offset, pn, expected, payload):
        self.conn, self.sealed, self.header, self.pn_offset = conn, sealed, header, pn_offset
        self.pn, self.expected, self.payload = pn, expected, payload
        self.pn_len = len(header) - pn_offset
        assert self.pn_len == (header[0] & 3) + 1
        assert quic_ref.decode_pn(expected, int.from_bytes(header[pn_offset:], "big"), self.pn_len) == pn
        self.long = bool(header[0] & 0x80)
        self.want_gen = None  # set by Case
        self.damaged = False

    @property
    def pkt_len(self):
        return len(self.header) + len(self.payload) + 16


def short_packet(conn, sealed, pn, k, pn_offset=9, bit=None):
    """a 1-RTT packet of generation `sealed` (Key Phase bit sealed & 1 unless `bit` says otherwise), shape k of SHAPES; the
    reserved bits vary with k (they sit under header protection too)"""
    pn_len, L = SHAPES[k % len(SHAPES)]
    bit = sealed & 1 if bit is None else bit
    first = 0x40 | ((k & 3) << 3) | (bit << 2) | (pn_len - 1)
    header = bytes([first]) + CID[conn: conn + pn_offset - 1] + (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big")
    return Packet(conn, sealed, header, pn_offset, pn, max(0, pn - k % 3), PAYLOAD[k: k + L])


def long_packet(conn, sealed, pn, k, low_bits):
    """a Handshake packet (version 1) with the given reserved bits (0x0c) under the mask: 0x04 there is no Key Phase bit"""
    pn_len, L = SHAPES[k % len(SHAPES)]
    first = 0xe0 | (low_bits & 0x0c) | (pn_len - 1)
    body = CID[conn: conn + 17]
    header = bytes([first]) + body + (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big")
    return Packet(conn, sealed, header, 18, pn, pn, PAYLOAD[k: k + L])


class Case:
    """states: [gen, first_pn] per connection; stride: the bank stride"""

    def __init__(self, algo, states, stride, packets, nconn_material=None):
        self.algo, self.states, self.stride, self.packets = algo, [list(s) for s in states], stride, packets
        self.count = len(states)
        self.keys, self.hps = material(algo, nconn_material or len(states))
        for p in packets:
            gen, first_pn = self.states[p.conn]
            p.want_gen = model.choose(p.header[0], p.pn, gen, first_pn)

    def bank_generation(self, conn, bank):
        """the generation whose keys sit in bank `bank` of a connection: the one of gen - 1, gen, gen + 1 with that residue"""
        gen = self.states[conn][0]
        return next(g for g in (gen - 1, gen, gen + 1) if g % 3 == bank)  # (gen = 0: bank 2 is generation -1, never keyed)

    def slot_keys(self):
        """{slot: (key, iv)} of the three banks of every connection"""
        out = {}
        for c in range(self.count):
            for bank in range(3):
                g = self.bank_generation(c, bank)
                if g >= 0:
                    out[c + self.stride * bank] = self.keys[c][g]
        return out

    def sealed_generation(self, p):
        return self.bank_generation(p.conn, 0) if p.long else p.sealed

    def must_open(self, p):
        if p.damaged:
            return False
        return True if p.long else p.want_gen == p.sealed

    def want_slot(self, p):
        return model.slot(p.conn, self.stride, p.want_gen)

    def protected(self, p):
        key, iv = self.keys[p.conn][self.sealed_generation(p)]
        if p.damaged:  # a forger does not have the AEAD key; the header (Key Phase bit, packet number) reads as it wrote it
            key = stream("quic-phase-forged-key", len(key))
        return _protect(self.algo, key, iv, self.hps[p.conn], p.header, p.pn, p.payload)


@functools.lru_cache(maxsize=None)
def _protect(algo, key, iv, hp, header, pn, payload):
    return quic_ref.protect(algo, key, iv, hp, header, pn, payload)


NCONN, STRIDE = 130, 137
MID = 5000


def bank_states(nconn=NCONN):
    """gen in 0..5 (every residue of 3 with both parities), first_pn from {0, mid, UINT64_MAX}, all fifteen pairs with a
    previous generation and the three without"""
    return [[c % 6, (0, MID + c, U64)[(c // 6) % 3]] for c in range(nconn)]


@functools.lru_cache(maxsize=None)
def three_banks(algo):
    """130 connections; per connection packets of the current generation, of the next one (pn >= first_pn) and of the previous
    one (pn < first_pn) wherever the state allows them, every shape, shuffled so that neighbouring lanes take different banks:
    all must open"""
    states = bank_states()
    pk, k = [], 0
    for c, (gen, first_pn) in enumerate(states):
        base = MID + c if first_pn != U64 else 77 + c
        pk.append(short_packet(c, gen, base + 40 + c, k))                       # current
        k += 1
        if first_pn != U64 and first_pn != 0:
            pk.append(short_packet(c, gen, first_pn - 3, k))                    # current, reordered below first_pn
            k += 1
        if first_pn != U64 or gen == 0:  # next: pn >= first_pn (also == first_pn), or no previous generation to mistake it for
            pk.append(short_packet(c, gen + 1, (0 if first_pn == U64 else first_pn) + 9 * (c % 4), k))
            k += 1
        if gen > 0 and first_pn != 0:
            pk.append(short_packet(c, gen - 1, (first_pn - 1 - c % 5) if first_pn != U64 else (1 << 40) + c, k))  # previous
            k += 1
    random.Random(130).shuffle(pk)
    case = Case(algo, states, STRIDE, pk)
    assert all(case.must_open(p) for p in pk)
    return case


@functools.lru_cache(maxsize=None)
def one_key_only(algo):
    """packets the single key tried must refuse: sealed under gen + 2 (the bit says gen), and sealed under the previous
    generation on a pn >= first_pn (the rule says gen + 1); a few good packets among them"""
    states = bank_states(36)
    pk, k = [], 3
    for c, (gen, first_pn) in enumerate(states):
        pk.append(short_packet(c, gen + 2, MID + 100 + c, k))
        k += 1
        if gen > 0 and first_pn != U64:
            pk.append(short_packet(c, gen - 1, first_pn + c % 3, k))
            k += 1
        if c % 4 == 0:
            pk.append(short_packet(c, gen, MID + 200 + c, k))
            k += 1
    random.Random(36).shuffle(pk)
    case = Case(algo, states, STRIDE, pk, NCONN)
    assert sum(case.must_open(p) for p in pk) == 9 and len(pk) > 60
    return case


@functools.lru_cache(maxsize=None)
def long_and_short(algo):
    """Handshake packets with every value of the reserved bits (0x04 among them) between 1-RTT packets, one call: the long
    ones are opened under the connection's own slot with NO_GEN"""
    states = bank_states(24)
    pk = []
    for c, (gen, first_pn) in enumerate(states):
        pk.append(long_packet(c, None, 10 + c, c, 0x04 * (1 + c % 3)))
        pk.append(short_packet(c, gen + (c % 2 if first_pn != U64 or gen == 0 else 0), MID + 300 + c, c + 5))
    case = Case(algo, states, STRIDE, pk, NCONN)
    assert all(case.must_open(p) for p in pk) and all(p.want_gen == model.NO_GEN for p in pk if p.long)
    return case


@functools.lru_cache(maxsize=None)
def commit_case(algo):
    """three_banks' packets, with every next-generation packet of the connections c % 7 == 3 forged (sealed without the
    key: a forged update must not advance them) and none from the connections c % 7 == 5 (their reordered current-generation packets
    lower first_pn), and a Handshake packet on every tenth connection"""
    base = three_banks(algo)
    pk = []
    for i, q in enumerate(base.packets):
        if q.want_gen == base.states[q.conn][0] + 1 and q.conn % 7 == 5:
            continue
        p = Packet(q.conn, q.sealed, q.header, q.pn_offset, q.pn, q.expected, q.payload)
        if q.want_gen == base.states[q.conn][0] + 1 and q.conn % 7 == 3:
            p.damaged = True
        pk.append(p)
        if q.conn % 10 == 0 and q.want_gen == base.states[q.conn][0]:
            pk.append(long_packet(q.conn, None, 3 + q.conn, i, 0x04))
    return Case(algo, base.states, STRIDE, pk)


def commit_inputs(case):
    """what the commit sees of a case whose packets are all selected: (connections, results, packet numbers, gen_out)"""
    return ([p.conn for p in case.packets], [len(p.payload) if case.must_open(p) else U64 for p in case.packets],
            [p.pn for p in case.packets], [p.want_gen for p in case.packets])


def after_commit(algo, states):
    """fresh packets for the states a commit left: per connection one of the current generation, one of the previous one
    (below first_pn) and one of the next one (at or above it) wherever the state allows them: all must open"""
    pk, k = [], 7
    for c, (g, first_pn) in enumerate(states):
        pk.append(short_packet(c, g, (first_pn if first_pn != U64 else 900) + 11, k))
        k += 1
        if g > 0 and first_pn != 0:
            pk.append(short_packet(c, g - 1, first_pn - 1 if first_pn != U64 else 12345, k))
            k += 1
        if first_pn != U64 or g == 0:
            pk.append(short_packet(c, g + 1, (first_pn if first_pn != U64 else 0) + 20, k))
            k += 1
    random.Random(131).shuffle(pk)
    case = Case(algo, states, STRIDE, pk, NCONN)
    assert all(case.must_open(p) for p in pk)
    return case


@functools.lru_cache(maxsize=None)
def seam_case(algo, nconn):
    """one 1-RTT packet per connection, for the commit's scan seam: every fifth connection updates, every tenth of the rest
    sends a forged update, the others a current-generation packet that lowers first_pn on every third of them"""
    states = [[c % 2, 100] for c in range(nconn)]
    pk = []
    for c in range(nconn):
        g = states[c][0]
        if c % 5 == 0 or c in (nconn - 1, 2046, 2047):
            pk.append(short_packet(c, g + 1, 100 + c % 7, 2 * 4 + c % 2))
        elif c % 10 == 3:
            pk.append(short_packet(c, g + 1, 100 + c % 7, 2 * 4 + c % 2))
            pk[-1].damaged = True
        else:
            pk.append(short_packet(c, g, 90 + 20 * (c % 3), 2 * 4 + c % 2))
    random.Random(nconn).shuffle(pk)
    return Case(algo, states, nconn + 1, pk)


MARK_PER_THREAD, MARK_WG = 4, 256  # csrc/internal.h QPH_MARK_PER_THREAD; the mark kernel's workgroup


@functools.lru_cache(maxsize=None)
def grouping_case(algo):
    """bulk traffic of four connections in buffer order (not shuffled), laid out for the groupings of the commit's mark pass.
    With 1 500 packets thread t of 512 takes packets t, t + 512 and t + 1024, so a wave of threads sees three rows:
      waves 0, 1  connection 0, current generation, in every row: folded twice, then reduced; the lowest packet number sits in
                  row 1 at lane 37 of wave 1; every eleventh packet of row 2 is forged with a still lower number, and lanes
                  60..63 of wave 1 hold forged packets only (lanes that hold nothing beside lanes that do)
      waves 2, 3  connection 1, next generation, a Handshake packet in every ninth place; the lowest in row 2, lane 13 of wave 3
      wave 4      connection 0, then 1, then 2: the place changes twice (two flushes), the wave ends on one place
      wave 5      connections 2 (current) and 3 (next) in alternating lanes, numbers falling: two places in one wave
      wave 6      connection 0 again, lanes 10..20 forged in every row
      wave 7      connection 1 in rows 0 and 1; row 2 ends at lane 27 with connection 0: two places again"""
    states = [[2, 10 ** 6], [1, 100], [4, 10 ** 6], [3, 50]]

    def forged(conn, sealed):
        p = short_packet(conn, sealed, 3, 8)
        p.damaged = True
        return p

    pk = []
    for j in range(1500):
        row, t = divmod(j, 512)
        w, lane = divmod(t, 64)
        if w in (0, 1):
            if (w == 1 and lane >= 60) or (row == 2 and t % 11 == 5):
                pk.append(forged(0, 2))
            else:
                pk.append(short_packet(0, 2, 7 if (row, t) == (1, 64 + 37) else 20000 + j, 8 + j % 2))
        elif w in (2, 3):
            pk.append(long_packet(1, None, 5, 8, 0x04) if j % 9 == 4 else
                      short_packet(1, 2, 150 if (row, t) == (2, 192 + 13) else 500 + j, 8 + j % 2))
        elif w == 4:
            pk.append((short_packet(0, 2, 20000 + j, 8), short_packet(1, 2, 500 + j, 9), short_packet(2, 4, 9500 + j, 8))[row])
        elif w == 5:
            pk.append(short_packet(2, 4, 9000 - j, 8) if lane % 2 == 0 else short_packet(3, 4, 9000 - j, 9))
        elif w == 6:
            pk.append(forged(0, 2) if 10 <= lane <= 20 else short_packet(0, 2, 20000 + j, 9))
        else:
            pk.append(short_packet(0, 2, 20000 + j, 8) if row == 2 else short_packet(1, 2, 500 + j, 9))
    return Case(algo, states, 5, pk, NCONN)


def mark_paths(case):
    """which groupings the mark pass goes through for a case whose packets are all selected, from its geometry (thread t of T
    = 256 * ceil(m / (256 * MARK_PER_THREAD)) takes packets t, t + T, ...; the device has more workgroups than that): counts of
    folds (a lane's successive packets with one place), of flushes (the place changed), and of waves that end with one place
    held by several lanes ("reduce"), of those with lanes that hold nothing ("partial"), and with two places or more ("split")"""
    conns, res, pns, gens = commit_inputs(case)
    m = len(conns)
    T = MARK_WG * -(-m // (MARK_WG * MARK_PER_THREAD))
    out = dict(fold=0, flush=0, reduce=0, partial=0, split=0, low_lanes=set())
    final = []
    for t in range(T):
        at, low = None, U64
        for j in range(t, m, T):
            g = case.states[conns[j]][0]
            if res[j] == U64 or gens[j] == model.NO_GEN or gens[j] not in (g, g + 1):
                continue
            place = (conns[j], gens[j] - g)
            if place == at:
                out["fold"] += 1
                low = min(low, pns[j])
            else:
                out["flush"] += at is not None
                at, low = place, pns[j]
        final.append((at, low))
    for w in range(0, T, 64):
        held = [(lane, at, low) for lane, (at, low) in enumerate(final[w: w + 64]) if at is not None]
        places = {at for _, at, _ in held}
        if len(places) > 1:
            out["split"] += 1
        elif len(held) > 1:
            out["reduce"] += 1
            out["partial"] += len(held) < 64
            out["low_lanes"].add(min(held, key=lambda h: h[2])[0])
    return out
