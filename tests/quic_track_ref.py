"""A plain-Python model of received-packet-number tracking (include/ptls_hip.h 2k), written from the rule's text alone: a
space's accepted numbers are a Python set, a window is turned into such a set and back by arithmetic on integers, and nothing
here shares a bit trick with hsig-picotls_amd/csrc/quic_track.h.

A space's state is [next, window]: next = the largest accepted packet number + 1 (0: none yet); bit k of window says that
packet number next - 1 - k has been accepted.  The table holds the spaces of connection c at [3 c + s]."""
U64 = (1 << 64) - 1
NONE, NEW, DUPLICATE, TOO_OLD = 0, 1, 2, 3
WINDOW = 64
INITIAL, ZERO_RTT, HANDSHAKE, RETRY, ONE_RTT, VERSION_NEGOTIATION, UNKNOWN_VERSION, NO_TYPE = range(8)
SPACE_OF = {INITIAL: 0, HANDSHAKE: 1, ZERO_RTT: 2, ONE_RTT: 2}


def accepted(next_, window):
    """the packet numbers a state remembers"""
    return {next_ - 1 - k for k in range(WINDOW) if (window // (2 ** k)) % 2 == 1}


def window_of(next_, numbers):
    """the window of the numbers among `numbers` that lie within WINDOW behind next_"""
    return sum(2 ** (next_ - 1 - pn) for pn in set(numbers) if 0 <= next_ - 1 - pn < WINDOW)


def tracked(conn, type_, result, count):
    return result != U64 and conn < count and type_ in SPACE_OF


def track(spaces, expected, count, conns, types, results, pns):
    """One call over the selected packets (conns[j], types[j], results[j], pns[j]) in selected order.  spaces (a list of
    [next, window], 3 * count of them) and expected (a list of integers of any length, or None) are moved on in place.
    Returns (the verdicts, the touched connections in ascending order)."""
    before = [list(s) for s in spaces]
    verdicts, new, seen = [], {}, set()
    for conn, type_, result, pn in zip(conns, types, results, pns):
        if not tracked(conn, type_, result, count):
            verdicts.append(NONE)
            continue
        place = 3 * conn + SPACE_OF[type_]
        next_, window = before[place]
        if pn < next_ and next_ - 1 - pn >= WINDOW:
            verdicts.append(TOO_OLD)
        elif pn < next_ and pn in accepted(next_, window):
            verdicts.append(DUPLICATE)
        elif (place, pn) in seen:
            verdicts.append(DUPLICATE)
        else:
            seen.add((place, pn))
            new.setdefault(place, []).append(pn)
            verdicts.append(NEW)
    for place, numbers in new.items():
        next_, window = before[place]
        after = max(next_, 1 + max(numbers))
        spaces[place] = [after, window_of(after, accepted(next_, window) | set(numbers))]
        if expected is not None and place < len(expected):
            expected[place] = after
    return verdicts, sorted({place // 3 for place in new})
