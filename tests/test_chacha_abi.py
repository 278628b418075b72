"""CPU tests of the ChaCha20-Poly1305 surface of libptls_hip.so: the library exports the new entry points and objects, the
two algorithm objects carry the field values of ptls_minicrypto_chacha20poly1305 / ptls_minicrypto_chacha20
(lib/cifra/chacha20.c:97-113), and ptls_hip_keyset_new_algo checks its arguments without touching a device."""
import ctypes

import ptls_hip

FUNCTIONS = ("ptls_hip_keyset_new_algo", "ptls_hip_keyset_algo", "ptls_hip_chacha20poly1305_seal_batch",
             "ptls_hip_chacha20poly1305_open_batch", "ptls_hip_chacha20poly1305_seal_batch_supp", "ptls_hip_chacha20_mask_batch",
             "ptls_hip_batch_set_chacha_lanes", "ptls_hip_batch_chacha_lanes")


class Algo(ctypes.Structure):  # ptls_aead_algorithm_t, include/picotls.h:499-560 (layout: tests/test_abi.py)
    _fields_ = [("name", ctypes.c_char_p), ("conf", ctypes.c_uint64), ("integ", ctypes.c_uint64), ("ctr", ctypes.c_void_p),
                ("ecb", ctypes.c_void_p), ("key_size", ctypes.c_size_t), ("iv_size", ctypes.c_size_t),
                ("tag_size", ctypes.c_size_t), ("fixed_iv", ctypes.c_size_t), ("record_iv", ctypes.c_size_t),
                ("bits", ctypes.c_uint8), ("align_bits", ctypes.c_uint8), ("context_size", ctypes.c_size_t),
                ("setup", ctypes.c_void_p)]


class Cipher(ctypes.Structure):  # ptls_cipher_algorithm_t, include/picotls.h:408-415
    _fields_ = [("name", ctypes.c_char_p), ("key_size", ctypes.c_size_t), ("block_size", ctypes.c_size_t),
                ("iv_size", ctypes.c_size_t), ("context_size", ctypes.c_size_t), ("setup", ctypes.c_void_p)]


def test_library_exports_the_chacha_symbols():
    L = ptls_hip.lib()
    for name in FUNCTIONS:
        assert hasattr(L, name), name
        assert name in ptls_hip.SIGNATURES, name
    for name in ("ptls_hip_chacha20poly1305", "ptls_hip_chacha20"):
        assert ctypes.c_char.in_dll(L, name) is not None
        assert name in ptls_hip.DATA_SYMBOLS
    assert (ptls_hip.ALGO_AESGCM, ptls_hip.ALGO_CHACHA20POLY1305) == (1, 2)


def test_algorithm_objects_mirror_minicrypto():
    L = ptls_hip.lib()
    a, c = Algo.in_dll(L, "ptls_hip_chacha20poly1305"), Cipher.in_dll(L, "ptls_hip_chacha20")
    # lib/cifra/chacha20.c:100-113 with include/picotls.h:87-92, :239-240
    assert a.name == b"CHACHA20-POLY1305"
    assert (a.conf, a.integ) == ((1 << 64) - 1, 1 << 36)
    assert (a.key_size, a.iv_size, a.tag_size) == (32, 12, 16)
    assert (a.fixed_iv, a.record_iv, a.bits & 1, a.align_bits) == (12, 0, 0, 0)
    assert a.ctr == ctypes.addressof(c) and a.ecb is None
    assert a.context_size >= 80 and a.setup
    # lib/cifra/chacha20.c:97-99
    assert (c.name, c.key_size, c.block_size, c.iv_size) == (b"CHACHA20", 32, 1, 16)
    assert c.context_size >= 32 and c.setup
    # and field for field against the reference's own objects, where the reference build at hand holds them
    from oracle_lib import REF_SO, Ref
    if Ref.available:
        ref = ctypes.CDLL(REF_SO)
        try:
            b, d = Algo.in_dll(ref, "ptls_minicrypto_chacha20poly1305"), Cipher.in_dll(ref, "ptls_minicrypto_chacha20")
        except ValueError:  # oracle/_ref is fusion + the AES minicrypto files: the literal values above are the check
            return
        fields = ("name", "conf", "integ", "key_size", "iv_size", "tag_size", "fixed_iv", "record_iv", "bits", "align_bits")
        assert [getattr(a, f) for f in fields] == [getattr(b, f) for f in fields]
        assert (a.ecb is None) == (b.ecb is None)
        assert [getattr(c, f) for f in ("name", "key_size", "block_size", "iv_size")] == \
               [getattr(d, f) for f in ("name", "key_size", "block_size", "iv_size")]


def test_keyset_new_algo_argument_checks():
    """bad arguments fail with a message before any device call (a NULL engine among them, so this runs without a GPU)"""
    L = ptls_hip.lib()
    for algo, key_size, nslots in ((ptls_hip.ALGO_CHACHA20POLY1305, 32, 4),  # NULL engine
                                   (ptls_hip.ALGO_AESGCM, 16, 4),
                                   (0, 32, 4), (3, 32, 4)):
        assert L.ptls_hip_keyset_new_algo(None, algo, key_size, nslots) is None
        assert "bad arguments" in ptls_hip.last_error()
    # argument order of the checks: the algorithm's key size and the slot count, whatever the engine is.  A non-NULL engine
    # pointer is never dereferenced before they pass.
    fake = ctypes.create_string_buffer(256)
    for key_size, nslots in ((16, 4), (0, 4), (33, 4), (32, 0), (32, 1 << 32)):
        assert L.ptls_hip_keyset_new_algo(ctypes.addressof(fake), ptls_hip.ALGO_CHACHA20POLY1305, key_size, nslots) is None
        assert "keyset_new_algo: bad arguments" in ptls_hip.last_error()
    assert L.ptls_hip_keyset_algo(None) == ptls_hip.EINVAL
    assert L.ptls_hip_batch_set_chacha_lanes(None, 4) == ptls_hip.EINVAL
    assert L.ptls_hip_batch_chacha_lanes(None) == ptls_hip.EINVAL
