"""The plain-Python model of packet-number tracking (tests/quic_track_ref.py) against hand-written statements, case by case:
every number below was worked out from the rule's text (include/ptls_hip.h 2k), not from the model.  Then the shared case
generator (tests/quic_track_cases.py) against the properties its users rely on."""
import quic_track_cases as gen
import quic_track_ref as model

U64 = model.U64
NONE, NEW, DUP, OLD = model.NONE, model.NEW, model.DUPLICATE, model.TOO_OLD
ALL = (1 << 64) - 1
T = model.ONE_RTT


def one(next_, window, pns, results=None, count=1, conn=0, type_=T):
    """a call on one space of connection 0: (verdicts, [next, window] after, touched, expected[2] after)"""
    spaces = [[5, 1], [6, 1], [next_, window]] + [[9, 1]] * (3 * (count - 1))
    expected = [1111, 2222, 3333]
    results = [20] * len(pns) if results is None else results
    verdicts, touched = model.track(spaces, expected, count, [conn] * len(pns), [type_] * len(pns), results, pns)
    assert spaces[0] == [5, 1] and spaces[1] == [6, 1] and expected[:2] == [1111, 2222]
    return verdicts, spaces[2], touched, expected[2]


def test_shifts():
    # the state: 100 accepted, and 98: next 101, bits 0 and 2
    assert one(101, 0b101, [100]) == ([DUP], [101, 0b101], [], 3333)                      # shift 0: nothing new
    assert one(101, 0b101, [99]) == ([NEW], [101, 0b111], [0], 101)                       # shift 0, a hole filled
    assert one(101, 0b101, [101]) == ([NEW], [102, 0b1011], [0], 102)                     # shift 1
    assert one(101, 0b101, [163]) == ([NEW], [164, 1 | 1 << 63], [0], 164)                # shift 63: 100 is at bit 63, 98 fell out
    assert one(101, 0b101, [164]) == ([NEW], [165, 1], [0], 165)                          # shift 64: the old window is gone
    assert one(101, 0b101, [165]) == ([NEW], [166, 1], [0], 166)                          # shift 65
    assert one(101, 0b101, [100 + (1 << 40)]) == ([NEW], [101 + (1 << 40), 1], [0], 101 + (1 << 40))
    assert one(101, ALL, [163]) == ([NEW], [164, 1 | ALL << 63 & ALL], [0], 164)


def test_the_back_of_the_window():
    # next 1000: bit 63 is packet 936, packet 935 is behind the window
    assert one(1000, 1, [936]) == ([NEW], [1000, 1 | 1 << 63], [0], 1000)
    assert one(1000, 1 | 1 << 63, [936]) == ([DUP], [1000, 1 | 1 << 63], [], 3333)
    assert one(1000, 1, [935]) == ([OLD], [1000, 1], [], 3333)
    assert one(1000, ALL, [935, 0]) == ([OLD, OLD], [1000, ALL], [], 3333)
    # too old is judged against the state before the call: 936 is still inside although the call moves next on
    assert one(1000, 1, [2000, 936]) == ([NEW, NEW], [2001, 1], [0], 2001)                # accepted, and not remembered
    assert one(2001, 1, [936]) == ([OLD], [2001, 1], [], 3333)                            # its replay: refused


def test_duplicates():
    assert one(50, 0b1001, [46]) == ([DUP], [50, 0b1001], [], 3333)                       # against the old window
    assert one(50, 0b1001, [47, 47]) == ([NEW, DUP], [50, 0b1101], [0], 50)               # in the call: two copies
    assert one(50, 0b1001, [60, 60, 60]) == ([NEW, DUP, DUP], [61, 1 | 0b1001 << 11], [0], 61)  # three copies
    assert one(50, 0b1001, [60, 47, 60, 47]) == ([NEW, NEW, DUP, DUP], [61, 1 | 1 << 13 | 0b1001 << 11], [0], 61)
    assert one(200, 1, [100, 100]) == ([OLD, OLD], [200, 1], [], 3333)                    # a duplicate of a too-old number
    # a failed copy in front does not make the real one a duplicate
    assert one(50, 0b1001, [47, 47], [U64, 20]) == ([NONE, NEW], [50, 0b1101], [0], 50)


def test_an_empty_space():
    assert one(0, 0, [0]) == ([NEW], [1, 1], [0], 1)
    assert one(0, 0, [7]) == ([NEW], [8, 1], [0], 8)
    assert one(0, 0, [7, 0, 7, 3]) == ([NEW, NEW, DUP, NEW], [8, 0b10010001], [0], 8)
    assert one(0, 0, [100, 3]) == ([NEW, NEW], [101, 1], [0], 101)                        # 3 is 97 behind: not remembered
    top = (1 << 62) - 1
    assert one(0, 0, [top]) == ([NEW], [1 << 62, 1], [0], 1 << 62)
    assert one(1 << 62, 1, [top, top - 1]) == ([DUP, NEW], [1 << 62, 0b11], [0], 1 << 62)


def test_a_bulk_batch_is_all_new():
    n = 262144
    verdicts, after, touched, expected = one(1000, ALL, list(range(1000, 1000 + n)))
    assert verdicts == [NEW] * n and after == [1000 + n, ALL] and touched == [0] and expected == 1000 + n


def test_forged_packets_change_nothing():
    # the failed packet carries the largest number of the call
    assert one(101, 0b101, [101, (1 << 62) - 1, 102], [20, U64, 20]) == ([NEW, NONE, NEW], [103, 0b10111], [0], 103)
    assert one(101, 0b101, [1 << 61], [U64]) == ([NONE], [101, 0b101], [], 3333)


def test_connections_at_the_end_of_the_table():
    spaces = [[0, 0] for _ in range(6)]
    expected = [7] * 9
    verdicts, touched = model.track(spaces, expected, 2, [1, 2, 0xffffffff, 1], [T] * 4, [20] * 4, [4, 4, 4, 5])
    assert verdicts == [NEW, NONE, NONE, NEW] and touched == [1]
    assert spaces == [[0, 0]] * 5 + [[6, 0b11]] and expected == [7] * 5 + [6] + [7] * 3


def test_spaces_stay_apart_and_types_without_a_space():
    spaces = [[10, 1], [10, 1], [10, 1]]
    types = [model.INITIAL, model.HANDSHAKE, model.ONE_RTT, model.ZERO_RTT, model.RETRY, model.VERSION_NEGOTIATION,
             model.UNKNOWN_VERSION, model.NO_TYPE]
    verdicts, touched = model.track(spaces, None, 1, [0] * 8, types, [20] * 8, [12] * 8)
    assert verdicts == [NEW, NEW, NEW, DUP, NONE, NONE, NONE, NONE]                       # 0-RTT and 1-RTT share a space
    assert spaces == [[13, 0b1001]] * 3 and touched == [0]
    # a short expected-pn table: only the elements it has are written
    spaces, expected = [[10, 1], [10, 1], [10, 1]], [0, 0]
    model.track(spaces, expected, 1, [0] * 3, types[:3], [20] * 3, [12] * 3)
    assert expected == [13, 13]


def test_the_generator():
    g = gen.grid()
    assert len(g) > 10000
    shifts, backs, verdicts = set(), set(), set()
    for next_, window, pk in g:
        assert window == 0 if next_ == 0 else window & 1 and window < 1 << min(next_, 64)
        for _, pn in pk:
            assert 0 <= pn < 1 << 62
            (backs if pn < next_ else shifts).add(next_ - 1 - pn if pn < next_ else pn + 1 - next_)
    assert {1, 63, 64, 65, 1 << 40} <= shifts and {0, 1, 62, 63, 64, 65} <= backs
    for part in range(3):
        call = gen.case_list(part)
        v, touched, after, exp = call.want([0] * call.expected_len)
        verdicts |= set(v)
        assert call.count == 130 and len(touched) > 60 and len(call.packets) > 600
        assert call.want([0] * call.expected_len, spaces=after)[0].count(NEW) == 0        # replayed: nothing is new twice
        same = call.permuted(5).want([0] * call.expected_len)
        assert same[1:] == (touched, after, exp) and sorted(same[0]) == sorted(v)
        assert after[21] == after[23] != call.spaces[21] and after[22][0] == 601          # connection 7's spaces
    assert verdicts == {NONE, NEW, DUP, OLD}
    bulk = gen.bulk_call()
    v, touched, after, _ = bulk.want()
    paths = gen.claim_paths(bulk)
    assert len(bulk.packets) == 4096 and touched == [0, 1] and after[2][1] == ALL and v.count(NEW) == 4096 - 44
    assert after[2][0] == 1000 + sum(1 for p in bulk.packets if p[1] == T and p[2] != U64 and p[0] == 0)
    assert paths["fold"] > 2500 and paths["flush"] >= 100 and paths["reduce"] >= 12 and paths["partial"] >= 1 and paths["split"] >= 2
    assert 37 in paths["top_lanes"]
    assert len(gen.spread_triples(gen.triples_call())) > 100
