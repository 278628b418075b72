#!/usr/bin/env python3
"""QUIC key derivation on the device (ptls_hip_keyset_set_quic_secrets / _set_quic_initial) next to what existed before it
and to the reference on one CPU core, in one process.

  python tools/bench_quic_keys.py [--count N] [--steps K] [--warmup W] [--ref-sample M]

Per cipher (aes128, aes256, chacha), N connections (default 65 536), wall time of the synchronous calls, median of K:

  quic_secrets   set_quic_secrets: three labels per secret, two keysets (AEAD + header protection) expanded
  tls_secrets    ptls_hip_keyset_set_secrets: the TLS 1.3 kernel, two labels per secret, one keyset expanded
  raw_two        ptls_hip_keyset_set of the AEAD keyset + of the header-protection keyset from raw keys: the upload and the
                 two key expansions alone, what a QUIC stack paid on the device before (after deriving on the CPU)
  raw_one        ptls_hip_keyset_set of the AEAD keyset alone (the expansion inside tls_secrets)
  quic_initial   (aes128 only) set_quic_initial of N connection IDs: 2 N slots in each keyset, 14 compression calls per slot
  raw_initial    the raw-key load of those 2 N slots in both keysets

and the reference's ptls_hkdf_expand_label (oracle/_ref, through ctypes; minicrypto's SHA-2) doing the same derivations on
one core: the three labels per secret, and for Initial keys Python's hmac for the Extract plus eight Expand-Labels per
connection, over a sample of M connections.  One JSON line per cipher.

The split of a call into its derivation kernel and its key-expansion kernels is read from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats -- python tools/bench_quic_keys.py ...): quic_derive_keys_kernel / quic_initial_keys_kernel
against keysetup_kernel / chacha_keysetup_kernel, and derive_traffic_keys_kernel for the TLS call.
"""
import argparse
import ctypes
import hashlib
import hmac
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hsig-picotls_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ptls_hip  # noqa: E402

CIPHERS = {"aes128": (ptls_hip.ALGO_AESGCM, 16, 32), "aes256": (ptls_hip.ALGO_AESGCM, 32, 48),
           "chacha": (ptls_hip.ALGO_CHACHA20POLY1305, 32, 32)}


def median_ms(call, steps, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()  # synchronous: the stream is synchronised before the call returns
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def rate(n, ms):
    return round(n / (ms * 1e-3))


def reference(hash_size, key_size, sample):
    """connections per second of the reference deriving key / iv / hp of a secret, and (SHA-256, 16-byte keys) of Initial
    keys, on this core; None without oracle/_ref"""
    from oracle_lib import REF_SO
    if not os.path.exists(REF_SO):
        return None, None
    L = ctypes.CDLL(REF_SO)
    f = L.ref_hkdf_expand_label
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t]
    bits = 128 if hash_size == 32 else 256
    out = ctypes.create_string_buffer(48)

    def expand(secret, label, outlen):
        assert f(bits, out, outlen, secret, label, None, 0) == 0
        return out.raw[:outlen]

    def keys(secret):
        expand(secret, b"quic key", key_size), expand(secret, b"quic iv", 12), expand(secret, b"quic hp", key_size)

    secrets = [hashlib.sha384(b"%d" % i).digest()[:hash_size] for i in range(sample)]
    t0 = time.perf_counter()
    for s in secrets:
        keys(s)
    per_secret = sample / (time.perf_counter() - t0)
    per_initial = None
    if hash_size == 32 and key_size == 16:
        salt = ptls_hip.QUIC_V1_SALT
        t0 = time.perf_counter()
        for s in secrets:
            initial = hmac.new(salt, s[:8], hashlib.sha256).digest()
            keys(expand(initial, b"client in", 32)), keys(expand(initial, b"server in", 32))
        per_initial = sample / (time.perf_counter() - t0)
    return round(per_secret), per_initial and round(per_initial)


def run(eng, cipher, args):
    algo, ksz, hs = CIPHERS[cipher]
    n = args.count
    rng = np.random.default_rng(9001)
    secrets = rng.integers(0, 256, n * hs, dtype=np.uint8).tobytes()
    initial = cipher == "aes128"
    slots = 2 * n if initial else n
    raw_keys = rng.integers(0, 256, slots * ksz, dtype=np.uint8).tobytes()
    raw_ivs = rng.integers(0, 256, slots * 12, dtype=np.uint8).tobytes()
    ks, hp = ptls_hip.KeySet(eng, ksz, slots, algo=algo), ptls_hip.KeySet(eng, ksz, slots, algo=algo)
    m = lambda call: median_ms(call, args.steps, args.warmup)  # noqa: E731
    quic_ms = m(lambda: ks.set_quic_secrets(hp, 0, secrets, hs))
    tls_ms = m(lambda: ks.set_secrets(0, secrets, hs))
    raw_one_ms = m(lambda: ks.set(0, raw_keys[:n * ksz], raw_ivs[:n * 12]))
    raw_two_ms = m(lambda: (ks.set(0, raw_keys[:n * ksz], raw_ivs[:n * 12]), hp.set(0, raw_keys[:n * ksz], None)))
    out = dict(cipher=cipher, connections=n, hash_size=hs,
               quic_secrets=dict(ms=round(quic_ms, 3), conn_per_s=rate(n, quic_ms)),
               tls_secrets=dict(ms=round(tls_ms, 3), conn_per_s=rate(n, tls_ms)),
               raw_two=dict(ms=round(raw_two_ms, 3)), raw_one=dict(ms=round(raw_one_ms, 3)))
    if initial:
        # the C call on packed connection IDs (KeySet.set_quic_initial packs a Python list on every call)
        dcids = rng.integers(0, 256, n * ptls_hip.QUIC_DCID_STRIDE, dtype=np.uint8).tobytes()
        lens = bytes(8 + i % 13 for i in range(n))
        salt, stream = ptls_hip.QUIC_V1_SALT, torch.cuda.current_stream().cuda_stream
        ini_ms = m(lambda: ptls_hip._check(ptls_hip.lib().ptls_hip_keyset_set_quic_initial(
            ks.ptr, hp.ptr, 0, n, dcids, lens, salt, len(salt), ptls_hip.QUIC_LABELS_V1, stream), "keyset_set_quic_initial"))
        raw_ini_ms = m(lambda: (ks.set(0, raw_keys, raw_ivs), hp.set(0, raw_keys, None)))
        out["quic_initial"] = dict(ms=round(ini_ms, 3), conn_per_s=rate(n, ini_ms), slots=slots)
        out["raw_initial"] = dict(ms=round(raw_ini_ms, 3))
    ks.close()
    hp.close()
    per_secret, per_initial = reference(hs, ksz, args.ref_sample)
    out["reference_one_core"] = dict(secrets_conn_per_s=per_secret, initial_conn_per_s=per_initial, sample=args.ref_sample)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ref-sample", type=int, default=4096)
    ap.add_argument("--cipher", default="all", choices=list(CIPHERS) + ["all"])
    args = ap.parse_args()
    eng = ptls_hip.Engine(0)
    for cipher in (CIPHERS if args.cipher == "all" else [args.cipher]):
        run(eng, cipher, args)
    eng.close()


if __name__ == "__main__":
    main()
