"""The plain-Python parse reference (tests/quic_parse_ref.py) pinned against known answers: the packets of RFC 9001
Appendix A (the client Initial of A.2, the server Initial of A.3, the ChaCha20 short-header packet of A.5), the varint
examples of RFC 9000 §A.1, and the output layout with max_per_dgram and MORE."""
import quic_parse_ref as ref
from test_quic_ref import A5_PACKET


def test_varint_examples_of_rfc9000():
    assert ref.varint(bytes.fromhex("c2197c5eff14e88c"), 0) == (151288809941952652, 8)
    assert ref.varint(bytes.fromhex("9d7f3e7d"), 0) == (494878333, 4)
    assert ref.varint(bytes.fromhex("7bbd"), 0) == (15293, 2)
    assert ref.varint(bytes.fromhex("25"), 0) == (37, 1)
    assert ref.varint(bytes.fromhex("4025"), 0) == (37, 2)  # a non-minimal encoding decodes
    assert ref.varint(bytes.fromhex("ff7bbd"), 1) == (15293, 3)
    # bounds: the first byte, and every byte its width asks for
    assert ref.varint(b"", 0) is None and ref.varint(b"\x25", 1) is None
    assert ref.varint(bytes.fromhex("7b"), 0) is None
    assert ref.varint(bytes.fromhex("9d7f3e"), 0) is None
    assert ref.varint(bytes.fromhex("c2197c5eff14e8"), 0) is None


def test_rfc9001_a2_client_initial():
    d = bytes.fromhex("c300000001088394c8f03e5157080000449e00000002").ljust(1200, b"\xa5")
    w = ref.walk_packet(d, 0, 1)
    assert w == dict(status=ref.OK, type=ref.INITIAL, version=1, dcid_off=6, dcid_len=8, scid_off=15, scid_len=0, token_off=16,
                     token_len=0, pn_offset=18, pkt_len=1200)
    assert d[w["dcid_off"]: w["dcid_off"] + w["dcid_len"]] == bytes.fromhex("8394c8f03e515708")
    assert ref.walk_datagram(d, 0, 16, 1) == [(0, w, False)]
    # one byte short of what Length says
    assert ref.walk_packet(d[:-1], 0, 1)["status"] == ref.TRUNCATED


def test_rfc9001_a3_server_initial():
    d = bytes.fromhex("c1000000010008f067a5502a4262b50040750001").ljust(135, b"\x5a")
    w = ref.walk_packet(d, 0, 1)
    assert (w["status"], w["type"], w["version"]) == (ref.OK, ref.INITIAL, 1)
    assert (w["pn_offset"], w["pkt_len"]) == (18, 135)
    assert (w["dcid_off"], w["dcid_len"], w["scid_off"], w["scid_len"]) == (6, 0, 7, 8)
    assert d[w["scid_off"]: w["scid_off"] + w["scid_len"]] == bytes.fromhex("f067a5502a4262b5")
    assert (w["token_off"], w["token_len"]) == (16, 0)


def test_rfc9001_a5_short_header_at_the_limit():
    assert len(A5_PACKET) == 21
    w = ref.walk_packet(A5_PACKET, 0, 1)
    assert (w["status"], w["type"], w["pn_offset"], w["pkt_len"], w["dcid_off"], w["dcid_len"]) == (ref.OK, ref.ONE_RTT, 1, 21, 1, 0)
    short = ref.walk_packet(A5_PACKET[:-1], 0, 1)
    assert (short["status"], short["pn_offset"], short["pkt_len"]) == (ref.TOO_SHORT, 0, 20)
    # the same bytes with an 8-byte DCID expected: too short as well
    assert ref.walk_packet(A5_PACKET, 8, 1)["status"] == ref.TOO_SHORT


def test_v2_type_bits_and_other_versions():
    body = bytes([0]) + bytes([0]) + bytes([20]) + bytes(20)  # no DCID, no SCID, Length 20
    for bits, typ in enumerate((ref.RETRY, ref.INITIAL, ref.ZERO_RTT, ref.HANDSHAKE)):
        d = bytes([0xC0 | bits << 4]) + ref.V2.to_bytes(4, "big") + body
        assert ref.walk_packet(d, 0, 1)["type"] == typ
    for bits, typ in enumerate((ref.INITIAL, ref.ZERO_RTT, ref.HANDSHAKE, ref.RETRY)):
        d = bytes([0xC0 | bits << 4]) + ref.V1.to_bytes(4, "big") + body
        assert ref.walk_packet(d, 0, 1)["type"] == typ
    vn = ref.walk_packet(bytes([0x80]) + bytes(4) + bytes([255]) + bytes(255) + bytes([3, 1, 2, 3]) + bytes(8), 0, 1)
    assert (vn["status"], vn["type"], vn["dcid_len"], vn["scid_off"], vn["scid_len"], vn["pn_offset"]) == \
        (ref.OK, ref.VERSION_NEGOTIATION, 255, 262, 3, 0)
    unk = ref.walk_packet(bytes([0x80]) + bytes.fromhex("0a1a2a3a") + bytes([21]) + bytes(21) + bytes([0]), 0, 1)
    assert (unk["status"], unk["type"], unk["version"], unk["dcid_len"]) == (ref.OK, ref.UNKNOWN_VERSION, 0x0A1A2A3A, 21)
    bad = ref.walk_packet(bytes([0xC0]) + ref.V1.to_bytes(4, "big") + bytes([21]) + bytes(40), 0, 1)
    assert (bad["status"], bad["pn_offset"], bad["pkt_len"]) == (ref.BAD_CID_LEN, 0, 46)


def test_fixed_bit():
    d = bytes.fromhex("8300000001088394c8f03e5157080000449e00000002").ljust(1200, b"\xa5")
    assert ref.walk_packet(d, 0, 1)["status"] == ref.BAD_FIXED_BIT
    assert ref.walk_packet(d, 0, 0)["status"] == ref.OK
    assert ref.walk_packet(bytes([0x0C]) + A5_PACKET[1:], 0, 1)["status"] == ref.BAD_FIXED_BIT
    assert ref.walk_packet(bytes([0x0C]) + A5_PACKET[1:], 0, 0)["status"] == ref.OK
    # an unknown version's fixed bit is not this endpoint's to judge
    assert ref.walk_packet(bytes([0x80]) + bytes.fromhex("0a1a2a3a") + bytes(2), 0, 1)["status"] == ref.OK


def test_layout_max_per_dgram_and_more():
    a2 = bytes.fromhex("c300000001088394c8f03e5157080000449e00000002").ljust(1200, b"\xa5")
    a3 = bytes.fromhex("c1000000010008f067a5502a4262b50040750001").ljust(135, b"\x5a")
    buf = b"\xee" * 3 + a2 + a3 + A5_PACKET + b"\xee" * 2 + a3[:10]
    dgrams = [(3, 1200 + 135 + 21), (0, 0), (3 + 1356 + 2, 10)]
    m = ref.CidMap(4)
    m.set(bytes.fromhex("8394c8f03e515708"), 5)
    m.set(b"", 1)
    expected = list(range(1000, 1018))
    out = ref.parse_datagrams(buf, dgrams, 0, 16, 1, m, expected, 17)
    assert [(p["pkt_off"], p["pkt_len"], p["pn_offset"], p["data_off"], p["key"], p["hp_key"], p["pn"]) for p, _ in out] == [
        (3, 1200, 18, 22, 5, 5, 1015), (1203, 135, 18, 1222, 1, 1, 1003), (1338, 21, 1, 1340, 1, 1, 1005),
        (1361, 10, 0, 1362, ref.NO_CONN, ref.NO_CONN, 0)]
    assert [(f["dgram"], f["type"], f["status"], f["conn"], f["flags"]) for _, f in out] == [
        (0, ref.INITIAL, ref.OK, 5, 0), (0, ref.INITIAL, ref.OK, 1, 0), (0, ref.ONE_RTT, ref.OK, 1, 0),
        (2, ref.INITIAL, ref.TRUNCATED, ref.NO_CONN, 0)]
    # expected_count 16: connection 5's Initial space (index 15) still counts, 17 would be its 1-RTT space
    assert ref.parse_datagrams(buf, dgrams, 0, 16, 1, m, expected, 15)[0][0]["pn"] == 0
    two = ref.parse_datagrams(buf, dgrams, 0, 2, 1, None)
    assert [(f["dgram"], f["flags"], f["conn"]) for _, f in two] == [(0, 0, ref.NO_CONN), (0, ref.MORE, ref.NO_CONN),
                                                                     (2, 0, ref.NO_CONN)]
    one = ref.parse_datagrams(buf, dgrams[:1], 0, 3, 1, None)
    assert [f["flags"] for _, f in one] == [0, 0, 0]  # exactly max_per_dgram entries and nothing behind them: no MORE
