#!/usr/bin/env python3
"""ChaCha20-Poly1305 through the host pipelines next to AES-128-GCM, on records that start and end in pinned host memory:
one process, one set of buffers and descriptors, one clock.

  python tools/bench_chacha_host.py [--steps K] [--warmup W] [--shape tls16k|quic1350|short256|all] [--rounds R]

Shapes, 1 GiB of payload each:
  tls16k    65 536 records of 16 384 bytes on one key, 5-byte AAD
  quic1350  795 364 records of 1 350 bytes over 65 536 keys (record i uses key i % 65 536), 13-byte AAD
  short256  4 194 304 records of 256 bytes (four ChaCha blocks) over 65 536 keys, 13-byte AAD: the low end of the width rule
Configurations, timed one after another and the whole list R times (so the two ChaCha layouts alternate and every
configuration is seen early and late in the run):
  mapped transport, ChaCha: the block kernel (a lane per 64-byte block) and the runs kernel (contiguous 16 x lanes-byte runs
                            per instruction) at 4 / 16 / 64 lanes per record, alternating; and the automatic choice
  copy transport, ChaCha
  AES-128-GCM through its own pipeline on the same descriptors, mapped and copy
A step is one pipeline seal of the whole gibibyte and one open of what it sealed; both calls return synchronised, and the
host clock (perf_counter) around the pair gives the step's time.  W untimed warm-up steps, then K timed ones; GiB/s = 2 x
payload / step time.  Per configuration: the median, and the spread (min and max) of the K steps.  Before the timing of every
configuration one step is checked: every open result, and the recovered bytes of 2 048 records spread over the batch.
One JSON line per configuration and round.
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
SHAPES = {
    "tls16k": dict(n=1 << 16, L=16384, keys=1, aad=5),
    "quic1350": dict(n=(1 << 30) // 1350, L=1350, keys=1 << 16, aad=13),
    "short256": dict(n=1 << 22, L=256, keys=1 << 16, aad=13),
}
BLOCKS, RUNS = ptls_hip.CHACHA_LAYOUT_BLOCKS, ptls_hip.CHACHA_LAYOUT_RUNS


def pinned(nbytes):
    t = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    assert t.is_pinned()
    return t, t.numpy()


def run_shape(eng, name, cfg, args):
    n, L, nkeys, A = cfg["n"], cfg["L"], cfg["keys"], cfg["aad"]
    stride = (L + 16 + 15) & ~15
    recs = np.zeros(n, dtype=ptls_hip.RECORD_DTYPE)
    idx = np.arange(n, dtype=np.uint64)
    recs["in_off"] = recs["out_off"] = idx * np.uint64(stride)
    recs["aad_off"] = idx * np.uint64(16)
    recs["seq"] = idx // np.uint64(nkeys)
    recs["len"], recs["aad_len"] = L, A
    recs["key"] = (idx % np.uint64(nkeys)).astype(np.uint32)
    rng = np.random.default_rng(1305)
    size = n * stride + 16
    keep = [pinned(size) for _ in range(3)] + [pinned(n * 16 + 16), pinned(n * 8)]
    (h_pt, h_ct, h_out, h_aad), h_res = [k[1] for k in keep[:4]], keep[4][1].view(np.uint64)
    tile = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    for o in range(0, size, 1 << 20):
        h_pt[o: o + (1 << 20)] = np.roll(tile, o >> 20)[: min(1 << 20, size - o)]
    h_aad[:] = rng.integers(0, 256, len(h_aad), dtype=np.uint8)
    h_ct[:] = 0
    payload = float(n) * L
    keys = rng.integers(0, 256, nkeys * 32, dtype=np.uint8).tobytes()
    ivs = rng.integers(0, 256, nkeys * 12, dtype=np.uint8).tobytes()
    cks = ptls_hip.KeySet(eng, 32, nkeys, algo=ptls_hip.ALGO_CHACHA20POLY1305)
    cks.set(0, keys, ivs)
    aks = ptls_hip.KeySet(eng, 16, nkeys)
    aks.set(0, keys[: nkeys * 16], ivs)
    cpipe = ptls_hip.Pipeline(eng, args.slice_mib << 20, algo=ptls_hip.ALGO_CHACHA20POLY1305)
    apipe = ptls_hip.Pipeline(eng, args.slice_mib << 20)
    sample = np.unique(np.linspace(0, n - 1, 2048).astype(np.int64))
    rows_pt = h_pt[: n * stride].reshape(n, stride)
    rows_out = h_out[: n * stride].reshape(n, stride)

    configs = []
    for g in (4, 16, 64):
        configs.append(("chacha mapped blocks %d" % g, cpipe, cks, ptls_hip.TRANSPORT_MAPPED, g, BLOCKS))
        configs.append(("chacha mapped runs %d" % g, cpipe, cks, ptls_hip.TRANSPORT_MAPPED, g, RUNS))
    configs.append(("chacha mapped auto", cpipe, cks, ptls_hip.TRANSPORT_MAPPED, 0, 0))
    configs.append(("chacha copy", cpipe, cks, ptls_hip.TRANSPORT_COPY, 0, 0))
    configs.append(("aes128gcm mapped", apipe, aks, ptls_hip.TRANSPORT_MAPPED, None, None))
    configs.append(("aes128gcm copy", apipe, aks, ptls_hip.TRANSPORT_COPY, None, None))

    for rnd in range(args.rounds):
        for label, pipe, ks, transport, lanes, layout in configs:
            pipe.set_transport(transport)
            if lanes is not None:
                pipe.set_chacha_lanes(lanes, layout)

            def step():
                t0 = time.perf_counter()
                pipe.seal(ks, recs, h_pt, h_aad, h_ct)
                pipe.open(ks, recs, h_ct, h_aad, h_out, h_res)
                return time.perf_counter() - t0

            rows_out[sample, :L] = 0
            h_res[:] = 0
            step()
            assert pipe.last_transport == transport, label
            assert bool((h_res == L).all()), label + ": an open failed"
            assert np.array_equal(rows_out[sample, :L], rows_pt[sample, :L]), label + ": round trip differs"
            for _ in range(max(0, args.warmup - 1)):
                step()
            times = [step() for _ in range(args.steps)]
            rates = sorted(2 * payload / t / GIB for t in times)
            print(json.dumps(dict(shape=name, round=rnd, config=label, records=n, record_bytes=L, keys=nkeys, steps=args.steps,
                                  warmup=args.warmup, seal_open_gibps=round(float(np.median(rates)), 2),
                                  min_gibps=round(rates[0], 2), max_gibps=round(rates[-1], 2),
                                  step_ms=[round(t * 1e3, 2) for t in times])), flush=True)
    cpipe.close()
    apipe.close()
    cks.close()
    aks.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--slice-mib", type=int, default=64, help="the pipelines' slice_bytes (the mapped transport cuts 4 x that)")
    ap.add_argument("--shape", default="all", choices=["all"] + list(SHAPES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a gfx950 device"
    eng = ptls_hip.Engine(0)
    for name in (list(SHAPES) if args.shape == "all" else [args.shape]):
        run_shape(eng, name, SHAPES[name], args)
    eng.close()


if __name__ == "__main__":
    main()
