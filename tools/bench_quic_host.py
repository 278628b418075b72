#!/usr/bin/env python3
"""QUIC packet protection from and to pinned host memory through the host pipelines (ptls_hip_pipeline_quic_seal / _open),
next to what the pipelines could do for such packets before those calls existed, in one process on one set of buffers:

  python tools/bench_quic_host.py [--steps K] [--warmup W] [--mib M] [--slice-mib S]

The packets: M MiB (default 256) of 1 350-byte payloads under 13-byte short headers (pn_offset 9, pn_len 4), 1 379 bytes
each at a 1 392-byte stride, under one key and under 65 536 keys (packet i uses AEAD and header-protection slot i % 65 536),
for AES-128-GCM, AES-256-GCM and ChaCha20-Poly1305, on the copy and on the mapped transport.  Per configuration two rows:

  quic     pipeline.quic_seal (payloads -> protected packets, the caller's headers already in h_pkt) and pipeline.quic_open
           (protected packets -> unprotected headers in h_pkt, packet numbers, plaintext): all of RFC 9001 §5.3 and §5.4.
  records  pipeline.seal_supp + pipeline.open over the same bytes as records with host-known descriptors (AAD = the
           headers in a buffer of their own, the ciphertext where the packet's is, the masks into a host array): the record
           protection and the mask computation only.  Nothing applies a mask to a header, and the open is given packet-number
           lengths, offsets and nonces that a receiver does not have before it has removed header protection.  This is the
           comparison, not an alternative.

seal and open are timed apart: each call returns synchronised, and the host clock (perf_counter) around it gives its time.
W untimed warm-up steps (a step = one seal and one open), then K timed ones; GiB/s = payload bytes / time; per row the
median and the spread (min, max) of the K steps.  Before the timing of a row one step is checked: every open result, every
packet number (quic), and the recovered payloads of 2 048 packets spread over the list.  One JSON line per row.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hsig-picotls_amd"))
import ptls_hip  # noqa: E402

GIB = float(1 << 30)
L, PN_OFFSET, PN_LEN = 1350, 9, 4
HDR = PN_OFFSET + PN_LEN
PKT = HDR + L + 16
STRIDE = (PKT + 15) & ~15
CIPHERS = (("aes128gcm", ptls_hip.ALGO_AESGCM, 16), ("aes256gcm", ptls_hip.ALGO_AESGCM, 32),
           ("chacha20poly1305", ptls_hip.ALGO_CHACHA20POLY1305, 32))


def pinned(nbytes):
    t = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    assert t.is_pinned()
    return t, t.numpy()


def rates(times, payload):
    r = sorted(payload / t / GIB for t in times)
    return round(float(np.median(r)), 2), round(r[0], 2), round(r[-1], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mib", type=int, default=256, help="payload bytes of the packet list")
    ap.add_argument("--slice-mib", type=int, default=64, help="the pipelines' slice_bytes (the mapped transport cuts 4 x that)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a gfx950 device"
    eng = ptls_hip.Engine(0)
    n = (args.mib << 20) // L
    payload = float(n) * L
    idx = np.arange(n, dtype=np.uint64)
    rng = np.random.default_rng(9001)
    size = n * STRIDE + 16
    keep = [pinned(size) for _ in range(3)] + [pinned(n * 16 + 16) for _ in range(2)] + [pinned(n * 8) for _ in range(2)]
    h_pt, h_pkt, h_out, h_aad, h_mask = [k[1] for k in keep[:5]]
    h_res, h_pn = keep[5][1].view(np.uint64), keep[6][1].view(np.uint64)
    tile = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    for o in range(0, size, 1 << 20):
        h_pt[o: o + (1 << 20)] = np.roll(tile, o >> 20)[: min(1 << 20, size - o)]
    # the unprotected headers: a short-header first byte with pn_len 4, eight connection-ID bytes, the truncated packet number
    pns = idx + np.uint64(1 << 20)
    hdrs = rng.integers(0, 256, (n, HDR), dtype=np.uint8)
    hdrs[:, 0] = 0x40 | (PN_LEN - 1)
    for j in range(PN_LEN):
        hdrs[:, PN_OFFSET + j] = ((pns >> np.uint64(8 * (PN_LEN - 1 - j))) & np.uint64(0xff)).astype(np.uint8)
    rows_pkt = h_pkt[: n * STRIDE].reshape(n, STRIDE)
    rows_pt = h_pt[: n * STRIDE].reshape(n, STRIDE)
    rows_out = h_out[: n * STRIDE].reshape(n, STRIDE)
    h_aad[: n * 16].reshape(n, 16)[:, :HDR] = hdrs
    sample = np.unique(np.linspace(0, n - 1, 2048).astype(np.int64))

    for nkeys in (1, 1 << 16):
        slots = (idx % np.uint64(nkeys)).astype(np.uint32)
        pk_seal = np.zeros(n, dtype=ptls_hip.QUIC_PACKET_DTYPE)
        pk_seal["pkt_off"] = pk_seal["data_off"] = idx * np.uint64(STRIDE)
        pk_seal["pn"], pk_seal["pkt_len"], pk_seal["key"], pk_seal["hp_key"] = pns, PKT, slots, slots
        pk_seal["pn_offset"], pk_seal["pn_len"] = PN_OFFSET, PN_LEN
        pk_open = pk_seal.copy()
        pk_open["pn"] = pns - np.uint64(1)  # the receiver expects the packet before
        recs = np.zeros(n, dtype=ptls_hip.RECORD_DTYPE)
        recs["in_off"] = idx * np.uint64(STRIDE)
        recs["out_off"] = idx * np.uint64(STRIDE) + np.uint64(HDR)
        recs["aad_off"] = idx * np.uint64(16)
        recs["seq"], recs["len"], recs["aad_len"], recs["key"] = pns, L, HDR, slots
        orecs = recs.copy()
        orecs["in_off"], orecs["out_off"] = recs["out_off"], recs["in_off"]
        supp = np.zeros(n, dtype=ptls_hip.SUPP_DTYPE)
        supp["sample_off"] = idx * np.uint64(STRIDE) + np.uint64(PN_OFFSET + 4)
        supp["mask_off"], supp["hp_key"], supp["flags"] = idx * np.uint64(16), slots, ptls_hip.SUPP_ENABLE
        for cipher, algo, ksz in CIPHERS:
            ks = ptls_hip.KeySet(eng, ksz, nkeys, algo=algo)
            hp = ptls_hip.KeySet(eng, ksz, nkeys, algo=algo)
            ks.set(0, rng.integers(0, 256, nkeys * ksz, dtype=np.uint8).tobytes(), rng.integers(0, 256, nkeys * 12, dtype=np.uint8).tobytes())
            hp.set(0, rng.integers(0, 256, nkeys * ksz, dtype=np.uint8).tobytes(), None)
            pipe = ptls_hip.Pipeline(eng, args.slice_mib << 20, algo=algo)
            for transport, tname in ((ptls_hip.TRANSPORT_COPY, "copy"), (ptls_hip.TRANSPORT_MAPPED, "mapped")):
                pipe.set_transport(transport)

                def quic_step():
                    t0 = time.perf_counter()
                    pipe.quic_seal(ks, hp, pk_seal, h_pt, h_pkt)
                    t1 = time.perf_counter()
                    pipe.quic_open(ks, hp, pk_open, h_pkt, h_out, h_res, h_pn)
                    return t1 - t0, time.perf_counter() - t1

                def record_step():
                    t0 = time.perf_counter()
                    pipe.seal_supp(ks, hp, recs, supp, h_pt, h_aad, h_pkt, h_mask)
                    t1 = time.perf_counter()
                    pipe.open(ks, orecs, h_pkt, h_aad, h_out, h_res)
                    return t1 - t0, time.perf_counter() - t1

                for path, step in (("quic", quic_step), ("records", record_step)):
                    rows_pkt[:, :HDR] = hdrs  # the caller's headers (the quic open leaves them as they were)
                    rows_out[sample, :L] = 0
                    h_res[:] = 0
                    h_pn[:] = 0
                    step()
                    assert pipe.last_transport == transport, (cipher, tname, path)
                    assert bool((h_res == L).all()), (cipher, tname, path, "an open failed")
                    assert np.array_equal(rows_out[sample, :L], rows_pt[sample, :L]), (cipher, tname, path, "round trip differs")
                    if path == "quic":
                        assert np.array_equal(h_pn, pns), (cipher, tname, "packet numbers differ")
                        assert np.array_equal(rows_pkt[sample, :HDR], hdrs[sample]), (cipher, tname, "headers differ")
                    for _ in range(max(0, args.warmup - 1)):
                        step()
                    times = [step() for _ in range(args.steps)]
                    seal, open_ = rates([t[0] for t in times], payload), rates([t[1] for t in times], payload)
                    print(json.dumps(dict(cipher=cipher, keys=nkeys, transport=tname, path=path, packets=n, payload_bytes=L,
                                          packet_bytes=PKT, steps=args.steps, warmup=args.warmup, seal_gibps=seal[0],
                                          seal_min=seal[1], seal_max=seal[2], open_gibps=open_[0], open_min=open_[1],
                                          open_max=open_[2])), flush=True)
            pipe.close()
            ks.close()
            hp.close()
    eng.close()


if __name__ == "__main__":
    main()
