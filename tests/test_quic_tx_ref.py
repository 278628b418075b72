"""The plain-Python model of the send object (tests/quic_tx_ref.py; include/ptls_hip.h 2l) against hand-written statements:
RFC 9000 A.2's two examples, every boundary of the packet-number length, the refusals and their precedence, the runs, the key
banks, and the decoder of RFC 9000 A.3 on what was sent.  The shared cases (tests/quic_tx_cases.py) are checked for holding
what the other tests rely on."""
import pytest

import quic_ref
import quic_tx_cases as gen
import quic_tx_ref as model
from quic_tx_ref import Conn, NONE_ACKED, NO_CONN, PN, RANGE, SENT, SPLIT, U64

BIG = 1 << 40


def one(conn, length=20, n=1, pn_len=0, rx=None, in_len=BIG, buf_len=BIG, data_off=0, pkt_off=0):
    """n requests of one connection (0) with room everywhere"""
    reqs = [(data_off + j * length, pkt_off + j * 70000, 0, length) for j in range(n)]
    return model.seal([conn], reqs, 1, 1, 1, in_len, buf_len, pn_len, None if rx is None else [rx])


def test_rfc9000_a2_examples():
    assert model.pn_len(0xac5c02, 0xabe8b3) == 2  # "29,519 ... 16 bits"
    assert model.pn_len(0xace8fe, 0xabe8b3) == 3  # "a 24-bit packet number encoding is needed"
    o = one(Conn(next_pn=0xac5c02, largest_acked=0xabe8b3, dcid=b"\x01\x02"))
    assert o.status == [SENT] and o.headers == [bytes([0x41, 1, 2, 0x5c, 0x02])] and o.pkt_len == [1 + 2 + 2 + 20 + 16]
    o = one(Conn(next_pn=0xace8fe, largest_acked=0xabe8b3))
    assert o.headers == [bytes([0x42, 0xac, 0xe8, 0xfe])]


@pytest.mark.parametrize("k,below,at", [(7, 1, 2), (15, 2, 3), (23, 3, 4), (31, 4, 0)])
def test_num_unacked_boundaries(k, below, at):
    assert model.pn_len(1000 + (1 << k) - 1, 1000) == below and model.pn_len(1000 + (1 << k), 1000) == at
    # none acknowledged: num_unacked = pn + 1
    assert model.pn_len((1 << k) - 2, NONE_ACKED) == below and model.pn_len((1 << k) - 1, NONE_ACKED) == at
    o = one(Conn(next_pn=1000 + (1 << k) - 1, largest_acked=1000), n=2)
    assert o.status == [SENT, SENT if at else PN] and o.pn_out == [1000 + (1 << k) - 1, 1000 + (1 << k)]
    assert o.pkt_len == [17 + below + 20, 17 + at + 20 if at else 0]


def test_first_packet_and_the_end_of_the_numbers():
    o = one(Conn())
    assert o.status == [SENT] and o.pn_out == [0] and o.headers == [b"\x40\x00"]
    o = one(Conn(next_pn=(1 << 62) - 1, largest_acked=(1 << 62) - 2), n=3)
    assert o.status == [SENT, PN, PN] and o.pn_out == [(1 << 62) - 1, 1 << 62, (1 << 62) + 1] and o.conns[0].next_pn == (1 << 62) + 2
    o = one(Conn(next_pn=U64 - 1), n=3)  # the sums saturate
    assert o.status == [PN] * 3 and o.pn_out == [U64 - 1, U64, U64] and o.conns[0].next_pn == U64


def test_acknowledged_numbers_are_refused():
    assert one(Conn(next_pn=500, largest_acked=500)).status == [PN]
    o = one(Conn(next_pn=400, largest_acked=401), n=3)
    assert o.status == [PN, PN, SENT] and o.pn_out == [400, 401, 402] and o.pkt_len == [0, 0, 38]


@pytest.mark.parametrize("min_len", range(5))
def test_params_pn_len(min_len):
    o = one(Conn(next_pn=50, largest_acked=49), pn_len=min_len)
    want = max(1, min_len)
    assert o.status == [SENT] and o.headers[0] == bytes([0x40 | (want - 1)]) + (50).to_bytes(want, "big")
    # a range that needs three bytes is not shortened by a smaller minimum, and lengthened by a larger one
    assert model.pn_len(0xace8fe, 0xabe8b3, min_len) == max(3, min_len)
    assert model.pn_len(1000 + (1 << 31), 1000, min_len) == 0


def test_short_payloads():
    c = Conn(next_pn=50, largest_acked=49)
    assert one(c, length=2).status == [RANGE]                 # 1 + 2 < 4: the sample would leave the packet
    assert one(c, length=3).status == [SENT]
    o = one(c, length=2, pn_len=2)
    assert o.status == [SENT] and o.pkt_len == [1 + 2 + 2 + 16]
    assert one(c, length=0, pn_len=4).status == [SENT] and one(c, length=0, pn_len=3).status == [RANGE]


def test_packet_length_limit():
    c = Conn(next_pn=20, largest_acked=19, dcid=bytes(8))
    longest = 65535 - 1 - 8 - 1 - 16
    assert one(c, length=longest).pkt_len == [65535]
    assert one(c, length=longest + 1).status == [RANGE] and one(c, length=0xFFFFFFFF).status == [RANGE]


def test_dcid_lengths():
    for n in (0, 8, 20):
        o = one(Conn(dcid=bytes(range(1, n + 1))))
        assert o.status == [SENT] and o.headers[0] == b"\x40" + bytes(range(1, n + 1)) + b"\x00" and o.pkt_len == [1 + n + 1 + 36]
    assert one(Conn(dcid=bytes(20), dcid_len=21)).status == [RANGE]


def test_buffer_ends():
    c = Conn()
    assert one(c, in_len=20, buf_len=38).status == [SENT]
    assert one(c, in_len=19, buf_len=38).status == [RANGE] and one(c, in_len=20, buf_len=37).status == [RANGE]
    assert one(c, data_off=U64).status == [RANGE] and one(c, pkt_off=U64 - 3).status == [RANGE]
    assert one(c, data_off=5, in_len=25, pkt_off=7, buf_len=45).status == [SENT]


def test_runs_a_b_a():
    conns = [Conn(next_pn=10, largest_acked=9), Conn(next_pn=700, largest_acked=9)]
    reqs = [(0, 100 * j, c, 20) for j, c in enumerate([0, 0, 1, 0, 1, 1, 0])]
    o = model.seal(conns, reqs, 2, 2, 2, BIG, BIG)
    assert o.status == [SENT, SENT, SENT, SPLIT, SPLIT, SPLIT, SPLIT]
    assert o.pn_out == [10, 11, 700, U64, U64, U64, U64] and o.pkt_len[3:] == [0] * 4
    assert (o.conns[0].next_pn, o.conns[1].next_pn) == (12, 701)  # later runs touch nothing
    # refused requests consume their number
    o = model.seal(conns, [(0, 0, 0, 20), (0, 100, 0, 2), (0, 200, 0, 20)], 2, 2, 2, BIG, BIG)
    assert o.status == [SENT, RANGE, SENT] and o.pn_out == [10, 11, 12] and o.conns[0].next_pn == 13


def test_no_conn_bounds():
    conns = [Conn() for _ in range(6)]
    reqs = [(0, 100 * c, c, 20) for c in range(6)] + [(0, 900, 0xFFFFFFFF, 20)]
    for count, stride, hp, n in ((6, 6, 6, 6), (4, 6, 6, 4), (6, 3, 6, 3), (6, 6, 2, 2)):
        o = model.seal(conns, reqs, count, stride, hp, BIG, BIG)
        assert o.status == [SENT] * n + [NO_CONN] * (7 - n) and o.pn_out[n:] == [U64] * (7 - n)
        assert all(o.conns[c] == conns[c] for c in range(n, 6))


def test_precedence():
    bad = Conn(next_pn=9, largest_acked=9, dcid=bytes(20), dcid_len=21)  # PN and RANGE at once
    conns = [bad, Conn()]
    # NO_CONN before everything: an outside connection with a payload outside the input
    o = model.seal(conns, [(U64, U64, 2, 0xFFFFFFFF)], 2, 2, 2, 10, 10)
    assert o.status == [NO_CONN]
    # SPLIT before PN and RANGE; PN before RANGE
    o = model.seal(conns, [(0, 0, 0, 20), (0, 0, 1, 20), (U64, U64, 0, 2)], 2, 2, 2, BIG, BIG)
    assert o.status == [PN, SENT, SPLIT] and o.pn_out == [9, 0, U64]
    ok_pn = Conn(next_pn=10, largest_acked=9, dcid=bytes(20), dcid_len=21)
    assert model.seal([ok_pn], [(0, 0, 0, 20)], 1, 1, 1, BIG, BIG).status == [RANGE]


@pytest.mark.parametrize("gen", [0, 1, 2, 3, 0xFFFFFFFE])
def test_generations_choose_bank_and_bit(gen):
    conns = [Conn(), Conn(gen=gen, flags=1)]
    o = model.seal(conns, [(0, 0, 1, 20)], 2, 5, 2, BIG, BIG)
    assert o.slots == [1 + 5 * (gen % 3)] and o.headers[0][0] == 0x40 | 0x20 | (gen & 1) << 2 and o.conns[1].gen == gen


def test_receive_side_generation():
    for rx, used in ((None, 4), (3, 4), (4, 4), (5, 5), (7, 7)):
        o = one(Conn(gen=4), rx=rx)
        assert o.gens == [used] and o.conns[0].gen == used and o.headers[0][0] == 0x40 | (used & 1) << 2
    # a refused run still follows: the state holds the generation used
    o = one(Conn(gen=4, next_pn=5, largest_acked=5), rx=5)
    assert o.status == [PN] and o.conns[0].gen == 5 and o.conns[0].next_pn == 6


def _decodes(call):
    o = call.want()
    assert o.sent
    for j in o.sent:
        conn, h = call.conns[call.reqs[j][2]], o.headers[j]
        L = (h[0] & 3) + 1
        expected = 0 if conn.largest_acked == NONE_ACKED else conn.largest_acked + 1
        assert quic_ref.decode_pn(expected, int.from_bytes(h[-L:], "big"), L) == o.pn_out[j], (j, h.hex())
        assert len(h) == 1 + conn.dcid_len + L and o.pkt_len[j] == len(h) + call.reqs[j][3] + 16
    return o


@pytest.mark.parametrize("pn_len", range(5))
def test_case_list_decodes_and_covers(pn_len):
    call = gen.case_list(pn_len)
    o = _decodes(call)
    assert set(o.status) == {SENT, NO_CONN, SPLIT, PN, RANGE}
    assert {(o.headers[j][0] & 3) + 1 for j in o.sent} == set(range(max(1, pn_len), 5))
    assert max(o.pkt_len) <= 65535 and (pn_len > 2 or 65535 in o.pkt_len)  # (the longest payloads are sized for 1 and 2 bytes)
    assert {len(o.headers[j]) - (o.headers[j][0] & 3) - 2 for j in o.sent} == {0, 8, 20}
    assert {o.headers[j][0] & 0x24 for j in o.sent} == {0, 4, 0x20, 0x24} and {s // gen.STRIDE for s in o.slots if s is not None} == {0, 1, 2}
    # the last packet and the last payload end with their buffers
    assert o.status[-1] == SENT and call.reqs[-1][1] + o.pkt_len[-1] == call.buf_len and call.reqs[-1][0] + call.reqs[-1][3] == call.in_len
    # every connection's first run is numbered, and sent packets do not overlap
    touched = [c for c in range(gen.NCONN) if o.conns[c] != call.conns[c]]
    assert len(touched) == gen.NCONN
    areas = sorted((call.reqs[j][1], call.reqs[j][1] + o.pkt_len[j]) for j in o.sent)
    assert all(a[1] <= b[0] for a, b in zip(areas, areas[1:]))
    # a two-byte payload: refused with one-byte numbers, sent with a minimum of two
    short = [j for j, r in enumerate(call.reqs) if r[3] == 2 and o.status[j] in (SENT, RANGE) and r[2] < gen.NCONN]
    assert short and (any(o.status[j] == SENT for j in short) if pn_len >= 2 else any(o.status[j] == RANGE for j in short))


def test_case_list_with_receive_generations():
    call = gen.case_list(0, rx="mixed")
    o, plain = _decodes(call), gen.case_list(0).want()
    moved = [c for c in range(gen.NCONN) if o.conns[c].gen != call.conns[c].gen]
    assert len(moved) > 30 and all(o.conns[c].gen == call.rx_gens[c] > call.conns[c].gen for c in moved)
    assert o.status == plain.status and o.pn_out == plain.pn_out and o.headers != plain.headers


@pytest.mark.parametrize("call", [gen.sized_call(257), gen.one_run_call(600), gen.edges_call(), gen.many_runs_call(2049), gen.lengths_call()],
                         ids=["sized", "one-run", "edges", "many-runs", "lengths"])
def test_size_calls_send_everything(call):
    o = _decodes(call)
    assert o.status == [SENT] * len(call.reqs)
    for c in range(call.count):
        n = sum(1 for r in call.reqs if r[2] == c)
        assert o.conns[c].next_pn == call.conns[c].next_pn + n
