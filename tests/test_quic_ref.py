"""tests/quic_ref.py pinned to the RFCs' own values: the ChaCha20-Poly1305 short-header packet of RFC 9001 A.5 (packet
protection and header protection end to end), the AES header-protection mask of RFC 9001 A.2, and the packet-number decode
example of RFC 9000 A.3.  No GPU."""
import quic_ref

A5_KEY = bytes.fromhex("c6d98ff3441c3fe1b2182094f69caa2ed4b716b65488960a7a984979fb23e1c8")
A5_IV = bytes.fromhex("e0459b3474bdd0e44a41c144")
A5_HP = bytes.fromhex("25a282b9e82f06f21f488917a4fc8f1b73573685608597d0efcb076b0ab7a7a4")
A5_PN = 654360564
A5_HEADER = bytes.fromhex("4200bff4")
A5_PAYLOAD = bytes.fromhex("01")
A5_SAMPLE = bytes.fromhex("5e5cd55c41f69080575d7999c25a5bfb")
A5_MASK = bytes.fromhex("aefefe7d03")
A5_PACKET = bytes.fromhex("4cfe4189655e5cd55c41f69080575d7999c25a5bfb")


def test_rfc9001_a5_chacha_short_header():
    assert quic_ref.hp_mask("chacha", A5_HP, A5_SAMPLE)[:5] == A5_MASK
    pkt = quic_ref.protect("chacha", A5_KEY, A5_IV, A5_HP, A5_HEADER, A5_PN, A5_PAYLOAD)
    assert pkt == A5_PACKET
    assert pkt[1 + 4: 1 + 4 + 16] == A5_SAMPLE
    # received with the largest packet number so far one below: three packet-number bytes decode to the full value
    header, pn, pt, ok = quic_ref.unprotect("chacha", A5_KEY, A5_IV, A5_HP, A5_PACKET, 1, A5_PN)
    assert (header, pn, pt, ok) == (A5_HEADER, A5_PN, A5_PAYLOAD, True)
    # a damaged payload byte (the sample of this packet is its whole tag): the raw plaintext still comes back
    bad = A5_PACKET[:4] + bytes([A5_PACKET[4] ^ 0x10]) + A5_PACKET[5:]
    assert quic_ref.unprotect("chacha", A5_KEY, A5_IV, A5_HP, bad, 1, A5_PN) == (A5_HEADER, A5_PN, b"\x11", False)
    # the already-unprotected form (a re-submission)
    unprot = A5_HEADER + A5_PACKET[4:]
    assert quic_ref.unprotect("chacha", A5_KEY, A5_IV, A5_HP, unprot, 1, A5_PN, protected=False) == \
        (A5_HEADER, A5_PN, A5_PAYLOAD, True)


def test_rfc9001_a2_aes_mask():
    hp = bytes.fromhex("9f50449e04a0e810283a1e9933adedd2")
    sample = bytes.fromhex("d1b1c98dd7689fb8ec11d242b123dc9b")
    assert quic_ref.hp_mask("aes128", hp, sample)[:5] == bytes.fromhex("437b9aec36")
    # the A.2 header c300000001088394c8f03e5157080000449e00000002 (pn_offset 18, 4 packet-number bytes) becomes
    # c000000001088394c8f03e5157080000449e7b9aec34
    header = bytes.fromhex("c300000001088394c8f03e5157080000449e00000002")
    mask = quic_ref.hp_mask("aes128", hp, sample)
    assert quic_ref.apply_mask(header, 18, 4, mask) == bytes.fromhex("c000000001088394c8f03e5157080000449e7b9aec34")


def test_rfc9000_a3_decode():
    assert quic_ref.decode_pn(0xa82f30ea + 1, 0x9b32, 2) == 0xa82f9b32
    # the window edges around an expected value, each pn_len: a packet number within half a window decodes to itself
    for pn_len in (1, 2, 3, 4):
        win = 1 << (8 * pn_len)
        for expected in (0, 1, win // 2, win, (1 << 31) + 5, (1 << 32) + 7, (1 << 62) - 3):
            for pn in (expected - win // 2 + 1, expected - 1, expected, expected + 1, expected + win // 2):
                if 0 <= pn < (1 << 62):
                    assert quic_ref.decode_pn(expected, pn & (win - 1), pn_len) == pn, (pn_len, expected, pn)


def test_round_trip_every_algorithm():
    for k, algo in enumerate(quic_ref.ALGOS):
        ksz = quic_ref.KEY_SIZE[algo]
        key, hp, iv = bytes(range(ksz)), bytes(range(100, 100 + ksz)), bytes(range(50, 62))
        for pn_len in (1, 2, 3, 4):
            for first, pn_offset in ((0x40, 1), (0x44, 9), (0xc0, 18)):
                pn = (1 << 33) + 0x1234567 + k
                header = bytes([first | (pn_len - 1)]) + bytes(range(7, 7 + pn_offset - 1)) + \
                    (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big")
                payload = bytes(range(20, 20 + 4 - pn_len + 3))
                pkt = quic_ref.protect(algo, key, iv, hp, header, pn, payload)
                assert len(pkt) == len(header) + len(payload) + 16 and pkt[len(header):-16] != payload
                assert quic_ref.unprotect(algo, key, iv, hp, pkt, pn_offset, pn - 3) == (header, pn, payload, True)
