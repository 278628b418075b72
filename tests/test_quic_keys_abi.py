"""CPU tests of the QUIC key-derivation surface of libptls_hip.so (include/ptls_hip.h 2f): the library exports the three
entry points and the binding declares them, the header carries the two label macros, and the refusals that need no device
(a null keyset or buffer, `labels` other than 1 or 2) fail with PTLS_HIP_EINVAL and their message, behind keyset pointers
that are never dereferenced before those checks."""
import ctypes
import os

import ptls_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("ptls_hip_keyset_set_quic_secrets", "ptls_hip_keyset_update_quic_secrets", "ptls_hip_keyset_set_quic_initial")


def test_library_exports_the_quic_key_symbols():
    L = ptls_hip.lib()
    with open(os.path.join(ROOT, "include", "ptls_hip.h")) as f:
        header = f.read()
    for name in FUNCTIONS:
        assert hasattr(L, name), name
        assert name in ptls_hip.SIGNATURES, name
        assert name + "(" in header, name
    assert (ptls_hip.QUIC_LABELS_V1, ptls_hip.QUIC_LABELS_V2) == (1, 2)
    assert "#define PTLS_HIP_QUIC_LABELS_V1 1" in header and "#define PTLS_HIP_QUIC_LABELS_V2 2" in header
    # the v1 salt is documented, not built in: the caller passes it
    assert ptls_hip.QUIC_V1_SALT.hex() == "38762cf7f55934b34d179ae6a4c80cadccbb7f0a" and ptls_hip.QUIC_V1_SALT.hex() in header
    for name in ("set_quic_secrets", "update_quic_secrets", "set_quic_initial"):
        assert callable(getattr(ptls_hip.KeySet, name))


def test_refusals_without_a_device():
    L = ptls_hip.lib()
    fake = ctypes.create_string_buffer(512)  # stands for a keyset: never dereferenced before the checks below pass
    ks = ctypes.addressof(fake)
    secrets = ctypes.create_string_buffer(64)
    dcids, lens, salt = ctypes.create_string_buffer(20), ctypes.create_string_buffer(1), ptls_hip.QUIC_V1_SALT

    def refused(rc, msg):
        assert rc == ptls_hip.EINVAL, msg
        assert msg in ptls_hip.last_error(), (msg, ptls_hip.last_error())

    for args in ((None, ks, 0, 1, secrets, 32, 1, None), (ks, None, 0, 1, secrets, 32, 1, None), (ks, ks, 0, 1, None, 32, 1, None)):
        refused(L.ptls_hip_keyset_set_quic_secrets(*args), "keyset_set_quic_secrets: null keyset or secrets")
    for args in ((None, 0, 1, secrets, 32, 1, None), (ks, 0, 1, None, 32, 1, None)):
        refused(L.ptls_hip_keyset_update_quic_secrets(*args), "keyset_update_quic_secrets: null keyset or secrets")
    for hole in range(5):
        args = [ks, ks, dcids, lens, salt]
        args[hole] = None
        refused(L.ptls_hip_keyset_set_quic_initial(args[0], args[1], 0, 1, args[2], args[3], args[4], len(salt), 1, None),
                "keyset_set_quic_initial: null keyset, connection IDs or salt")
    for labels in (0, 3, -1):
        refused(L.ptls_hip_keyset_set_quic_secrets(ks, ks, 0, 1, secrets, 32, labels, None),
                "keyset_set_quic_secrets: labels must be")
        refused(L.ptls_hip_keyset_update_quic_secrets(ks, 0, 1, secrets, 32, labels, None),
                "keyset_update_quic_secrets: labels must be")
        refused(L.ptls_hip_keyset_set_quic_initial(ks, ks, 0, 1, dcids, lens, salt, len(salt), labels, None),
                "keyset_set_quic_initial: labels must be")
    # count > 2^32 - 1 and the salt length are refused before the keysets are looked at, too
    refused(L.ptls_hip_keyset_set_quic_secrets(ks, ks, 0, 1 << 32, secrets, 32, 1, None), "above 2^32 - 1")
    refused(L.ptls_hip_keyset_update_quic_secrets(ks, 0, 1 << 32, secrets, 32, 2, None), "above 2^32 - 1")
    refused(L.ptls_hip_keyset_set_quic_initial(ks, ks, 0, 1 << 32, dcids, lens, salt, len(salt), 1, None), "above 2^32 - 1")
    for salt_len in (0, 65):
        refused(L.ptls_hip_keyset_set_quic_initial(ks, ks, 0, 1, dcids, lens, bytes(65), salt_len, 1, None), "outside 1..64")
    assert bytes(fake) == bytes(512)
