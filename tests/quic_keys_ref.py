"""Plain-Python QUIC key derivation (RFC 9001 §5.1, §5.2, §6; RFC 9369 §3.3): the expected values of the QUIC key tests.
HKDF comes from Python's hmac / hashlib; where the reference library is built (oracle/_ref), every Expand-Label is also
computed by the reference's ptls_hkdf_expand_label (oracle_lib.ref_hkdf_expand_label) and the two must agree.

hash_size is 32 (SHA-256) or 48 (SHA-384); v2 selects the "quicv2 " labels of RFC 9369."""
import functools
import hashlib
import hmac
import os

V1_SALT = bytes.fromhex("38762cf7f55934b34d179ae6a4c80cadccbb7f0a")  # RFC 9001 §5.2
V2_SALT = bytes.fromhex("0dede3def700a6db819381be6e269dcbf9bd2ed9")  # RFC 9369 §3.3.1
HASH = {32: hashlib.sha256, 48: hashlib.sha384}


@functools.lru_cache(maxsize=None)
def _ref():
    import oracle_lib
    return oracle_lib.ref_hkdf_expand_label if os.path.exists(oracle_lib.REF_SO) else None


def have_reference():
    return _ref() is not None


def hkdf_extract(salt, ikm, hash_size=32):
    return hmac.new(salt, ikm, HASH[hash_size]).digest()


def expand_label(secret, label, outlen, check=True):
    """HKDF-Expand-Label(secret, label, "", outlen) with outlen <= the hash size (one HMAC)"""
    hash_size = len(secret)
    assert outlen <= hash_size and len(label) <= 12
    info = outlen.to_bytes(2, "big") + bytes([6 + len(label)]) + b"tls13 " + label + b"\0"
    out = hmac.new(secret, info + b"\x01", HASH[hash_size]).digest()[:outlen]
    if check and have_reference():
        assert _ref()(128 if hash_size == 32 else 256, secret, label, outlen) == out, label
    return out


def prefix(v2):
    return b"quicv2 " if v2 else b"quic "


def keys(secret, key_size, v2=False, check=True):
    """(key, iv, hp) of a traffic secret"""
    p = prefix(v2)
    return (expand_label(secret, p + b"key", key_size, check), expand_label(secret, p + b"iv", 12, check),
            expand_label(secret, p + b"hp", key_size, check))


def update(secret, v2=False, check=True):
    """the next generation's secret (the key update)"""
    return expand_label(secret, prefix(v2) + b"ku", len(secret), check)


def initial_secrets(salt, dcid, check=True):
    """(client, server) Initial secrets of a client Destination Connection ID"""
    initial = hkdf_extract(salt, dcid)
    return expand_label(initial, b"client in", 32, check), expand_label(initial, b"server in", 32, check)
