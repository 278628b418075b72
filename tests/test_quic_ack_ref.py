"""The plain-Python model of the ACK-frame call (tests/quic_ack_ref.py; include/ptls_hip.h 2m) against byte strings written
by hand from RFC 9000 §19.3 and §16, and against the decoder of tests/quic_ack_cases.py, which reads a frame as a peer would:
what it returns must be exactly the accepted set, or with truncation exactly the newest 1 + max_ranges runs."""
import pytest

import quic_ack_cases as gen
import quic_ack_ref as model
from quic_ack_ref import EMPTY, NO_CONN, OK, STATE

U64 = gen.U64
ALT = gen.ALTERNATING
H = bytes.fromhex


def test_varints():
    want = {0: "00", 63: "3f", 64: "4040", 16383: "7fff", 16384: "80004000", (1 << 30) - 1: "bfffffff", 1 << 30: "c000000040000000",
            (1 << 62) - 1: "ffffffffffffffff", 37: "25", 15293: "7bbd", 494878333: "9d7f3e7d", 151288809941952652: "c2197c5eff14e88c"}
    for v, h in want.items():  # (the last four are RFC 9000 A.1's examples)
        assert model.varint(v) == H(h)
        assert gen.read_varint(H(h), 0) == (v, len(h) // 2)


def test_hand_written_frames():
    f = model.frame
    # next = 1: packet number 0 alone
    assert f(1, 1, 0, 31) == H("02 00 00 00 00")
    # a full window: 64 numbers below next, one range
    assert f(64, U64, 0, 31) == H("02 3f 00 00 3f")
    assert f(65, U64, 0, 31) == H("02 4040 00 00 3f")
    # a single bit
    assert f(1000, 1, 25, 31) == H("02 43e7 19 00 00")
    # 0b1011 under next = 10: numbers 9, 8 and 6; one gap of one number
    assert f(10, 0b1011, 5, 31) == H("02 09 05 01 01 00 00")
    # bits 0 and 63 under next = 100: 99 and 36; 62 numbers between them
    assert f(100, 1 | 1 << 63, 0, 31) == H("02 4063 00 01 00 3d 00")
    # alternating bits: 31 further ranges of one number behind gaps of one; 81 bytes with an 8-byte largest and delay
    long = f(1 << 62, ALT, (1 << 62) - 1, 31)
    assert long == H("02 ffffffffffffffff ffffffffffffffff 1f 00") + H("00 00") * 31 and len(long) == model.ACK_MAX == 81
    # ... the shortest there is has 5
    assert len(f(1, 1, 0, 0)) == 5


def test_stray_bits_count_for_nothing():
    """bits at k >= next name no packet number: the frame is the one of the window without them"""
    for n, w in gen.stray_bits():
        clean = w & ((1 << n) - 1)
        assert clean != w and model.frame(n, w, 7, 31) == model.frame(n, clean, 7, 31)
        assert model.accepted(n, w) == model.accepted(n, clean) and min(model.accepted(n, w)) >= 0
    assert model.frame(3, U64, 0, 31) == H("02 02 00 00 02")
    assert model.frame(1, U64, 0, 31) == H("02 00 00 00 00")
    assert model.frame(2, 0b101, 0, 31) == H("02 01 00 00 00")  # bit 2 would be packet number -1


@pytest.mark.parametrize("value", [63, 64, 16383, 16384, (1 << 30) - 1, 1 << 30, (1 << 62) - 1])
def test_largest_and_delay_at_every_varint_edge(value):
    size = len(model.varint(value))
    assert size == (1 if value < 64 else 2 if value < 16384 else 4 if value < 1 << 30 else 8)
    a = model.frame(value + 1, 0b101, 0, 31)
    assert a == b"\x02" + model.varint(value) + H("00 01 00 00 00") and len(a) == 1 + size + 1 + 2 + 2
    b = model.frame(9, 1, value, 31)
    assert b == H("02 08") + model.varint(value) + H("00 00") and gen.decode(b)[:2] == (8, value)


def test_max_ranges():
    n = 1 << 20
    full = model.frame(n, ALT, 0, 31)
    assert len(full) == 1 + 4 + 1 + 2 + 62
    for keep, want_r in ((0, 0), (1, 1), (30, 30), (31, 31), (32, 31), (0xFFFFFFFF, 31)):
        f = model.frame(n, ALT, 0, keep)
        assert f[6] == want_r and len(f) == 8 + 2 * want_r and f[7:] == full[7: 7 + 1 + 2 * want_r]
        _, _, ranges, end = gen.decode(f)
        assert end == len(f) and ranges == [(n - 1 - 2 * i, n - 1 - 2 * i) for i in range(want_r + 1)]
    # a window with three runs cut to the newest two
    assert model.frame(20, 0b1100110011, 0, 1) == H("02 13 00 01 01 01 01")


def test_status_and_precedence():
    s = model.status
    assert s(5, 5, 9, 1) == NO_CONN and s(0xFFFFFFFF, 5, 9, 1) == NO_CONN and s(4, 5, 9, 1) == OK
    assert s(0, 5, 0, 0) == EMPTY and s(0, 5, 0, U64) == EMPTY
    assert s(0, 5, 1 << 62, 1) == OK and s(0, 5, (1 << 62) + 1, 1) == STATE and s(0, 5, U64, U64) == STATE
    assert s(0, 5, 9, 0) == STATE and s(0, 5, 9, U64 - 1) == STATE
    # NO_CONN before EMPTY before STATE
    assert s(5, 5, 0, 0) == NO_CONN and s(5, 5, (1 << 62) + 1, 0) == NO_CONN and s(0, 5, 0, 2) == EMPTY
    out = model.ack([[0, 0], [9, 1], [9, 2]] * 2, 2, 1, [0, 2, 1, 1], ack_delay=3, in_off=100, pkt_base=7, pkt_stride=50)
    assert out.status == [OK, NO_CONN, OK, OK] and out.frame_len == [5, 0, 5, 5] and out.frame_off == [0, 5, 5, 10]
    assert out.bytes == H("02 08 03 00 00") * 3 and out.reqs == [(100, 7, 0, 5), (105, 57, 1, 5), (110, 107, 1, 5)]
    out = model.ack([[0, 0], [9, 1], [9, 2]] * 2, 2, 2, [0, 1], ack_delay=3)
    assert out.status == [STATE, STATE] and out.bytes == b"" and out.reqs == [] and out.frame_off == [0, 0]


def test_the_decoder_returns_the_accepted_set():
    entries = gen.grid() + gen.stray_bits() + gen.random_entries(3000, seed=5)
    seen_ok = 0
    for n, w in entries:
        if model.status(0, 1, n, w) != OK:
            continue
        seen_ok += 1
        for delay, keep in ((0, 31), ((1 << 62) - 1, 32), (64, 0), (16384, 1), (63, 5)):
            f = model.frame(n, w, delay, keep)
            assert 5 <= len(f) <= model.ACK_MAX
            largest, got_delay, ranges, end = gen.decode(f)
            assert end == len(f) and largest == n - 1 and got_delay == delay
            all_runs = model.runs(model.accepted(n, w))
            assert ranges == all_runs[:1 + min(keep, 31)]
            if keep >= 31:
                assert gen.acknowledged(ranges) == model.accepted(n, w)
            assert len(f) == 1 + len(model.varint(n - 1)) + len(model.varint(delay)) + 2 + 2 * (len(ranges) - 1)
    assert seen_ok > 3000
