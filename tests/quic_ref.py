"""Plain-Python QUIC packet protection (RFC 9001 §5.3, §5.4; RFC 9000 Appendix A.3): the expected bytes of every QUIC test
here.  AES-GCM and the AES header-protection mask go through the CPU oracle (oracle_lib.Oracle: seal, open, aes_ecb),
ChaCha20-Poly1305 and the ChaCha20 mask through tests/chacha_ref.py.  The nonce is picotls's (static IV XOR the big-endian
packet number in bytes 4..11), which is RFC 9001 §5.3's.

algo is "aes128", "aes256" or "chacha"; the key sizes follow (16 / 32 / 32 bytes, header-protection keys alike)."""
import functools

import chacha_ref

ALGOS = ("aes128", "aes256", "chacha")
KEY_SIZE = {"aes128": 16, "aes256": 32, "chacha": 32}


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle_lib import Oracle
    return Oracle()


def decode_pn(expected, truncated, pn_len):
    """RFC 9000 A.3 DecodePacketNumber, with expected = largest_pn + 1 and pn_nbits = 8 * pn_len."""
    pn_win = 1 << (8 * pn_len)
    pn_hwin = pn_win // 2
    pn_mask = pn_win - 1
    candidate = (expected & ~pn_mask) | truncated
    if candidate <= expected - pn_hwin and candidate < (1 << 62) - pn_win:
        return candidate + pn_win
    if candidate > expected + pn_hwin and candidate >= pn_win:
        return candidate - pn_win
    return candidate


def hp_mask(algo, hp_key, sample):
    """the 16-byte header-protection block of a 16-byte sample (RFC 9001 §5.4.3, §5.4.4); QUIC uses the first 5 bytes"""
    assert len(sample) == 16 and len(hp_key) == KEY_SIZE[algo]
    if algo == "chacha":
        return chacha_ref.hp_mask(hp_key, sample)
    return _oracle().aes_ecb(hp_key, sample)


def first_byte_bits(first):
    return 0x0f if first & 0x80 else 0x1f


def aead_seal(algo, key, iv, pn, aad, pt):
    if algo == "chacha":
        return chacha_ref.seal(key, iv, pn, aad, pt)
    return _oracle().seal(key, iv, pn, aad, pt)


def aead_open(algo, key, iv, pn, aad, sealed):
    """(plaintext, ok): the plaintext is computed whether or not the tag matches"""
    if algo == "chacha":
        return chacha_ref.open_(key, iv, pn, aad, sealed)
    n, pt = _oracle().open(key, iv, pn, aad, sealed)
    return pt, n is not None


def apply_mask(header, pn_offset, pn_len, mask):
    """header (bytes, at least pn_offset + pn_len) with the first byte and the packet-number bytes XORed with the mask"""
    h = bytearray(header)
    h[0] ^= mask[0] & first_byte_bits(h[0])
    for j in range(pn_len):
        h[pn_offset + j] ^= mask[1 + j]
    return bytes(h)


def protect(algo, key, iv, hp_key, header, pn, payload):
    """the protected packet.  header = the unprotected header, truncated packet number included: its pn_len is
    (header[0] & 3) + 1 and the packet-number field is its last pn_len bytes."""
    pn_len = (header[0] & 3) + 1
    pn_offset = len(header) - pn_len
    assert pn_offset >= 1
    pkt = header + aead_seal(algo, key, iv, pn, header, payload)
    assert len(pkt) >= pn_offset + 4 + 16, "the sample would leave the packet"
    mask = hp_mask(algo, hp_key, pkt[pn_offset + 4: pn_offset + 20])
    return apply_mask(pkt[:len(header)], pn_offset, pn_len, mask) + pkt[len(header):]


def unprotect(algo, key, iv, hp_key, packet, pn_offset, expected_pn, protected=True):
    """(header, pn, plaintext, ok) of a received packet: header = the unprotected header (pn_offset + pn_len bytes), pn = the
    full packet number decoded against expected_pn (largest received + 1), plaintext = the raw decryption even when the tag
    fails (ok False).  protected=False: the header is already unprotected (a re-submission under another key)."""
    assert len(packet) >= pn_offset + 4 + 16
    first = packet[0]
    mask = hp_mask(algo, hp_key, packet[pn_offset + 4: pn_offset + 20]) if protected else bytes(16)
    first ^= mask[0] & first_byte_bits(first)
    pn_len = (first & 3) + 1
    header = apply_mask(packet[:pn_offset + pn_len], pn_offset, pn_len, mask)
    assert header[0] == first
    pn = decode_pn(expected_pn, int.from_bytes(header[pn_offset:], "big"), pn_len)
    pt, ok = aead_open(algo, key, iv, pn, header, packet[pn_offset + pn_len:])
    return header, pn, pt, ok
