"""Plain-Python ChaCha20, Poly1305 and the ChaCha20-Poly1305 AEAD of RFC 8439 (big integers, no dependencies): the
expected bytes of every ChaCha test here.  Also picotls's per-record nonce (ptls_aead__build_iv: static IV with bytes 4..11
XORed with the big-endian sequence number) and its ChaCha20 header-protection mask (do_init(sample) then 16 keystream
bytes: counter = LE32(sample[0:4]), nonce = sample[4:16]; RFC 9001 §5.4.4)."""
import struct

P1305 = (1 << 130) - 5
_M32 = 0xffffffff


def _rotl(v, n):
    return ((v << n) & _M32) | (v >> (32 - n))


def _qr(s, a, b, c, d):
    s[a] = (s[a] + s[b]) & _M32
    s[d] = _rotl(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & _M32
    s[b] = _rotl(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b]) & _M32
    s[d] = _rotl(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & _M32
    s[b] = _rotl(s[b] ^ s[c], 7)


def chacha20_block(key, counter, nonce):
    """RFC 8439 §2.3: the 64-byte keystream block `counter` of (32-byte key, 12-byte nonce)."""
    assert len(key) == 32 and len(nonce) == 12
    init = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + list(struct.unpack("<8I", key)) + [counter & _M32] + \
        list(struct.unpack("<3I", nonce))
    s = list(init)
    for _ in range(10):
        _qr(s, 0, 4, 8, 12)
        _qr(s, 1, 5, 9, 13)
        _qr(s, 2, 6, 10, 14)
        _qr(s, 3, 7, 11, 15)
        _qr(s, 0, 5, 10, 15)
        _qr(s, 1, 6, 11, 12)
        _qr(s, 2, 7, 8, 13)
        _qr(s, 3, 4, 9, 14)
    return struct.pack("<16I", *[(a + b) & _M32 for a, b in zip(s, init)])


def chacha20_xor(key, counter, nonce, data):
    """RFC 8439 §2.4: data XOR the keystream starting at block `counter`."""
    out = bytearray()
    for i in range(0, len(data), 64):
        ks = chacha20_block(key, counter + i // 64, nonce)
        out += bytes(a ^ b for a, b in zip(data[i:i + 64], ks))
    return bytes(out)


def clamp_r(r16):
    return int.from_bytes(r16, "little") & 0x0ffffffc0ffffffc0ffffffc0fffffff


def poly1305_mac(msg, key):
    """RFC 8439 §2.5: the 16-byte tag of msg under the 32-byte one-time key r || s."""
    assert len(key) == 32
    r = clamp_r(key[:16])
    s = int.from_bytes(key[16:], "little")
    acc = 0
    for i in range(0, len(msg), 16):
        blk = msg[i:i + 16]
        acc = (acc + int.from_bytes(blk + b"\x01", "little")) * r % P1305
    return ((acc + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def poly1305_key_gen(key, nonce):
    """RFC 8439 §2.6."""
    return chacha20_block(key, 0, nonce)[:32]


def _pad16(b):
    return b"\x00" * (-len(b) % 16)


def aead_encrypt(key, nonce, plaintext, aad):
    """RFC 8439 §2.8: ciphertext || tag."""
    otk = poly1305_key_gen(key, nonce)
    ct = chacha20_xor(key, 1, nonce, plaintext)
    mac = aad + _pad16(aad) + ct + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct))
    return ct + poly1305_mac(mac, otk)


def aead_decrypt(key, nonce, sealed, aad):
    """plaintext, or None when the tag does not match (the plaintext is computed either way: aead_decrypt_raw)."""
    pt, ok = aead_decrypt_raw(key, nonce, sealed, aad)
    return pt if ok else None


def aead_decrypt_raw(key, nonce, sealed, aad):
    assert len(sealed) >= 16
    ct, tag = sealed[:-16], sealed[-16:]
    otk = poly1305_key_gen(key, nonce)
    mac = aad + _pad16(aad) + ct + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct))
    return chacha20_xor(key, 1, nonce, ct), poly1305_mac(mac, otk) == tag


def record_nonce(iv, seq):
    """picotls's ptls_aead__build_iv (lib/picotls.c:6492-6506)."""
    assert len(iv) == 12
    s = struct.pack(">Q", seq & 0xffffffffffffffff)
    return iv[:4] + bytes(a ^ b for a, b in zip(iv[4:], s))


def seal(key, iv, seq, aad, plaintext):
    return aead_encrypt(key, record_nonce(iv, seq), plaintext, aad)


def open_(key, iv, seq, aad, sealed):
    return aead_decrypt_raw(key, record_nonce(iv, seq), sealed, aad)


class SharedOpen:
    """open_ for many cases that keep (key, nonce): block 0 (the one-time key) and the keystream, the slow part in plain
    Python, are computed once per (key, nonce) and shared; the Poly1305 tag is computed per case with poly1305_mac.  The
    results equal open_'s (tests/test_chacha_ref.py)."""

    def __init__(self):
        self._ks = {}  # (key, nonce) -> [one-time key, keystream bytearray from block 1]

    def open_(self, key, iv, seq, aad, sealed):
        assert len(sealed) >= 16
        nonce = record_nonce(iv, seq)
        ent = self._ks.get((key, nonce))
        if ent is None:
            ent = self._ks[(key, nonce)] = [poly1305_key_gen(key, nonce), bytearray()]
        ct, tag = sealed[:-16], sealed[-16:]
        while len(ent[1]) < len(ct):
            ent[1] += chacha20_block(key, 1 + len(ent[1]) // 64, nonce)
        pt = (int.from_bytes(ct, "little") ^ int.from_bytes(ent[1][:len(ct)], "little")).to_bytes(len(ct), "little")
        mac = aad + _pad16(aad) + ct + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct))
        return pt, poly1305_mac(mac, ent[0]) == tag


def hp_mask(hp_key, sample):
    """the 16 mask bytes of a 16-byte sample (QUIC uses the first 5)."""
    assert len(sample) == 16
    return chacha20_block(hp_key, struct.unpack("<I", sample[:4])[0], sample[4:])[:16]
