"""Plain-Python model of the receive key chosen by Key Phase bit and of the commit of key updates (include/ptls_hip.h 2j;
hsig-picotls_amd/csrc/quic_phase.h).  Written from the header's text; nothing here calls the library.

A connection's state is (gen, first_pn): the generation of its current receive keys, whose Key Phase bit is gen & 1, and the
lowest packet number opened under it (U64: none yet).  The keys of generation g of connection c live in slot
c + stride * (g % 3)."""
U64 = (1 << 64) - 1
NO_GEN = 0xFFFFFFFF


def choose(first, pn, gen, first_pn):
    """the generation a packet with unmasked first byte `first` and full packet number pn is opened under"""
    if first & 0x80:
        return NO_GEN
    bit = (first >> 2) & 1
    if bit == gen & 1:
        return gen
    if gen > 0 and pn < first_pn:
        return gen - 1
    return gen + 1


def slot(key, stride, gen_out):
    return key if gen_out == NO_GEN else key + stride * (gen_out % 3)


def limit(stride, count):
    """the key-slot bound of the select rule, in place of the keyset's slots"""
    return min(stride, count)


def commit(table, conns, results, pns, gens):
    """table: a list of [gen, first_pn] per connection, changed in place; conns / results / pns / gens: per selected packet,
    its connection, result, packet number and gen_out.  Returns the updated connections, ascending."""
    nxt, cur = {}, {}
    for c, r, pn, g in zip(conns, results, pns, gens):
        if c >= len(table) or r == U64 or g == NO_GEN:
            continue
        if g == table[c][0] + 1:
            nxt[c] = min(nxt.get(c, U64), pn)
        elif g == table[c][0]:
            cur[c] = min(cur.get(c, U64), pn)
    for c in nxt:
        table[c][0] += 1
        table[c][1] = nxt[c]
    for c in cur:
        if c not in nxt:
            table[c][1] = min(table[c][1], cur[c])
    return sorted(nxt)
