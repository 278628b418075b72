#!/usr/bin/env python3
"""Generate tests/golden/chacha20poly1305.json by RUNNING THE REFERENCE'S OWN ENGINE.

The reference engine is picotls's minicrypto backend: ptls_minicrypto_chacha20poly1305 and ptls_minicrypto_chacha20
(lib/cifra/chacha20.c over lib/chacha20poly1305.h and deps/cifra), reached through picotls's public AEAD API
(lib/picotls.c: ptls_aead_new_direct, ptls_cipher_new; the inline dispatchers ptls_aead_encrypt / ptls_aead_encrypt_s /
ptls_aead_decrypt of include/picotls.h are one indirect call through the context's vtable each and are made from here with
ctypes, as tests/plugin_driver.py does).  The oracle's reference build (oracle/_ref) holds no ChaCha code and stays as it
is, so this script compiles the reference's sources, unmodified and from where they lie, into a throw-away shared library
in a temporary directory OUTSIDE the repository and deletes it afterwards.  Only data is written: inputs are derived from
the documented generator below, outputs are what the reference computed.

  python3 tests/golden/make_chacha_golden.py /path/to/picotls-checkout

Contents: 200 records over the length / AAD-length grid of tests/test_gpu_chacha.py with seq in {0, 1, 2^32 - 1, 2^32,
2^64 - 1} and non-zero IVs (full ct || tag up to 256 bytes of output, SHA-256 above), and 32 header-protection masks made by
ptls_aead_encrypt_s with a ptls_minicrypto_chacha20 context as `supp` (samples inside the ciphertext and over the tag).
Every entry is also checked against tests/chacha_ref.py before the file is written.
"""
import ctypes as c
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import chacha_ref  # noqa: E402

LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1350, 16384, 16385]
# the per-G lengths 64 G - 1, 64 G, 64 G + 1, 128 G + 1, 3 * 64 G + 17 for G = 1, 4, 16, 64 (those not above)
for _g in (1, 4, 16, 64):
    for _l in (64 * _g - 1, 64 * _g, 64 * _g + 1, 128 * _g + 1, 3 * 64 * _g + 17):
        if _l not in LENS:
            LENS.append(_l)
LENS.append(1500)  # the plugin test's Ethernet-sized record
AADS = [0, 1, 5, 12, 13, 16, 17, 21]
SEQS = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1]
NRECORDS = 200
NMASKS = 32
FULL_OUTPUT_MAX = 256


def stream(tag, n):
    """the input generator: SHA-256 in counter mode over the ASCII tag"""
    out = bytearray()
    i = 0
    while len(out) < n:
        out += hashlib.sha256(b"%s/%d" % (tag.encode(), i)).digest()
        i += 1
    return bytes(out[:n])


def record_inputs(i):
    """record i of the fixture: (key, iv, seq, aad, plaintext)"""
    L = LENS[i % len(LENS)]
    A = AADS[(i // len(LENS) + i) % len(AADS)]
    seq = SEQS[(i // 3) % len(SEQS)]
    s = stream("chacha20poly1305-record-%d" % i, 32 + 12 + A + L)
    iv = bytes(b | 1 for b in s[32:44])  # non-zero in every byte
    return s[:32], iv, seq, s[44:44 + A], s[44 + A:]


def mask_inputs(j):
    """mask j: a record (as above, index 1000 + j, length >= 32) with a header-protection key and a sample offset"""
    L = [32, 33, 64, 100, 255, 1350, 1351, 4000][j % 8]
    A = AADS[j % len(AADS)]
    s = stream("chacha20poly1305-mask-%d" % j, 32 + 12 + 32 + A + L)
    iv = bytes(b | 1 for b in s[32:44])
    sample_off = [0, 1, 4, L - 16, L - 7, L - 1, L, 3][j % 8]  # L - 7 .. L: the sample covers the tag
    return s[:32], iv, SEQS[j % len(SEQS)], s[76:76 + A], s[76 + A:], s[44:76], sample_off


class Ctx(c.Structure):
    _fields_ = [(n, c.c_void_p) for n in ("algo", "dispose_crypto", "do_get_iv", "do_set_iv", "do_encrypt_init",
                                            "do_encrypt_update", "do_encrypt_final", "do_encrypt", "do_encrypt_v", "do_decrypt")]


class Supp(c.Structure):
    _fields_ = [("ctx", c.c_void_p), ("input", c.c_void_p), ("output", c.c_uint8 * 16)]


ENCRYPT = c.CFUNCTYPE(None, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_uint64, c.c_void_p, c.c_size_t, c.c_void_p)
DECRYPT = c.CFUNCTYPE(c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_uint64, c.c_void_p, c.c_size_t)


def build_reference(ref, tmp):
    cifra = os.path.join(ref, "deps", "cifra", "src")
    # lib/cifra/chacha20.c names ptls_minicrypto_sha256 (its cipher-suite object), which lib/cifra/aes128.c defines
    srcs = [os.path.join(ref, "lib", f) for f in ("cifra/chacha20.c", "cifra/aes128.c", "picotls.c", "hpke.c")] + \
           [os.path.join(cifra, f) for f in ("chacha20poly1305.c", "chacha20.c", "poly1305.c", "blockwise.c", "sha256.c",
                                             "sha512.c", "chash.c", "aes.c", "gcm.c", "gf128.c", "modes.c")]
    so = os.path.join(tmp, "libptls_minicrypto_chacha.so")
    subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-shared", "-w", "-I" + os.path.join(ref, "include"), "-I" + cifra,
                    "-I" + os.path.join(cifra, "ext"), "-o", so] + srcs, check=True)
    return so


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "lib", "cifra", "chacha20.c")):
        sys.exit(__doc__)
    tmp = tempfile.mkdtemp(prefix="chacha_golden_")
    try:
        lib = c.CDLL(build_reference(sys.argv[1], tmp))
        lib.ptls_aead_new_direct.restype = c.c_void_p
        lib.ptls_aead_new_direct.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p]
        lib.ptls_aead_free.argtypes = [c.c_void_p]
        lib.ptls_cipher_new.restype = c.c_void_p
        lib.ptls_cipher_new.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
        lib.ptls_cipher_free.argtypes = [c.c_void_p]
        aead = c.addressof(c.c_char.in_dll(lib, "ptls_minicrypto_chacha20poly1305"))
        cipher = c.addressof(c.c_char.in_dll(lib, "ptls_minicrypto_chacha20"))

        def seal(key, iv, seq, aad, pt, hp_key=None, sample_off=0):
            ctx = lib.ptls_aead_new_direct(aead, 1, key, iv)
            out = c.create_string_buffer(len(pt) + 16)
            supp, hp = None, None
            if hp_key is not None:
                hp = lib.ptls_cipher_new(cipher, 1, hp_key)
                supp = Supp(hp, c.addressof(out) + sample_off)
            ENCRYPT(Ctx.from_address(ctx).do_encrypt)(ctx, out, pt, len(pt), seq, aad, len(aad),
                                                      c.byref(supp) if supp is not None else None)
            lib.ptls_aead_free(ctx)
            if hp is not None:
                lib.ptls_cipher_free(hp)
            return out.raw, (bytes(supp.output) if supp is not None else None)

        def open_(key, iv, seq, aad, sealed):
            ctx = lib.ptls_aead_new_direct(aead, 0, key, iv)
            out = c.create_string_buffer(max(len(sealed), 1))
            n = DECRYPT(Ctx.from_address(ctx).do_decrypt)(ctx, out, sealed, len(sealed), seq, aad, len(aad))
            lib.ptls_aead_free(ctx)
            return None if n == (1 << 64) - 1 else out.raw[:n]

        # the reference's engine reproduces RFC 8439 §2.8.2 before anything is recorded
        rfc_key = bytes(range(0x80, 0xa0))
        rfc_nonce = bytes.fromhex("070000004041424344454647")
        rfc_pt = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, sunscreen "
                  b"would be it.")
        out, _ = seal(rfc_key, rfc_nonce, 0, bytes.fromhex("50515253c0c1c2c3c4c5c6c7"), rfc_pt)
        assert out[-16:].hex() == "1ae10b594f09e26a7e902ecbd0600691", out[-16:].hex()

        records = []
        for i in range(NRECORDS):
            key, iv, seq, aad, pt = record_inputs(i)
            out, _ = seal(key, iv, seq, aad, pt)
            assert open_(key, iv, seq, aad, out) == pt
            assert out == chacha_ref.seal(key, iv, seq, aad, pt), i
            e = dict(i=i, L=len(pt), A=len(aad), seq=seq, sha256=hashlib.sha256(out).hexdigest())
            if len(out) <= FULL_OUTPUT_MAX:
                e["out"] = out.hex()
            records.append(e)
        masks = []
        for j in range(NMASKS):
            key, iv, seq, aad, pt, hp_key, sample_off = mask_inputs(j)
            out, mask = seal(key, iv, seq, aad, pt, hp_key, sample_off)
            assert out == chacha_ref.seal(key, iv, seq, aad, pt)
            assert mask == chacha_ref.hp_mask(hp_key, out[sample_off:sample_off + 16]), j
            masks.append(dict(j=j, L=len(pt), A=len(aad), seq=seq, sample_off=sample_off, sha256=hashlib.sha256(out).hexdigest(),
                              mask=mask.hex()))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    doc = dict(
        source="picotls minicrypto: ptls_minicrypto_chacha20poly1305 / ptls_minicrypto_chacha20 (lib/cifra/chacha20.c) through "
               "ptls_aead_new_direct + do_encrypt (ptls_aead_encrypt / ptls_aead_encrypt_s); generator: "
               "tests/golden/make_chacha_golden.py",
        derivation="inputs: make_chacha_golden.record_inputs(i) / mask_inputs(j): SHA-256 counter stream over "
                   "'chacha20poly1305-record-<i>/<n>' = key(32) | iv(12, every byte | 1) | aad(A) | pt(L); masks: "
                   "'chacha20poly1305-mask-<j>/<n>' = key | iv | hp_key(32) | aad | pt.  out = ct || tag (hex, when <= 256 "
                   "bytes); sha256 = SHA-256(ct || tag); mask = the 16 bytes of supp.output",
        rfc8439_2_8_2_tag="1ae10b594f09e26a7e902ecbd0600691",
        records=records, masks=masks)
    path = os.path.join(HERE, "chacha20poly1305.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0)
    print("written:", path, os.path.getsize(path), "bytes,", len(records), "records,", len(masks), "masks")


if __name__ == "__main__":
    main()
