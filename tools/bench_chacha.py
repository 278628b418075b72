#!/usr/bin/env python3
"""ChaCha20-Poly1305 next to AES-128-GCM on the same shapes, in one process on one clock (device-resident batches).

  python tools/bench_chacha.py [--steps K] [--warmup W] [--shape tls16k|quic1350|all] [--lanes G] [--sweep-lanes]

Shapes (reduced counts of bench.py's c2 / c4 so a run takes seconds):
  tls16k    65 536 records of 16 384 bytes on one key, 5-byte AAD
  quic1350  1 048 576 records of 1 350 bytes over 65 536 keys (record i uses key i % 65 536), 13-byte AAD
Timing discipline of bench.py: W untimed warm-up steps (seal + open), a synchronize, then K steps; each step's seal and
open are bracketed by HIP events on the launch stream and the medians are reported, with the wall clock over all K steps
beside them.  GiB/s = payload bytes sealed + opened per second (2 x payload per step).  Every open result and every
recovered byte is checked once before the timing.  One JSON line per shape; --sweep-lanes adds the ChaCha kernel at every
lanes-per-record width.
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
    "quic1350": dict(n=1 << 20, L=1350, keys=1 << 16, aad=13),
}


def measure(step, steps, warmup, payload):
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for _ in range(warmup):
        step(stream, None)
    torch.cuda.synchronize()
    times = []
    t0 = time.perf_counter()
    for _ in range(steps):
        step(stream, ev)
        torch.cuda.synchronize()
        times.append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
    wall = time.perf_counter() - t0
    seal_ms = float(np.median([a for a, _ in times]))
    open_ms = float(np.median([b for _, b in times]))
    return dict(seal_gibps=round(payload / (seal_ms * 1e-3) / GIB, 1), open_gibps=round(payload / (open_ms * 1e-3) / GIB, 1),
                seal_open_gibps=round(2 * payload / ((seal_ms + open_ms) * 1e-3) / GIB, 1),
                seal_ms=round(seal_ms, 3), open_ms=round(open_ms, 3),
                wall_gibps=round(2 * payload * steps / wall / GIB, 1))


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
    d_pt = torch.empty(n * stride + 16, dtype=torch.uint8, device="cuda")
    d_ct = torch.zeros(n * stride + 16, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(n * stride + 16, dtype=torch.uint8, device="cuda")
    d_aad = torch.from_numpy(rng.integers(0, 256, n * 16 + 16, dtype=np.uint8)).cuda()
    d_res = torch.zeros(n, dtype=torch.int64, device="cuda")
    batch = ptls_hip.Batch(eng, recs)
    batch.fill(d_pt, 0x6368616368613230)
    torch.cuda.synchronize()
    payload = float(n) * L
    keys = rng.integers(0, 256, nkeys * 32, dtype=np.uint8).tobytes()
    ivs = rng.integers(0, 256, nkeys * 12, dtype=np.uint8).tobytes()
    out = dict(shape=name, records=n, record_bytes=L, keys=nkeys, aad_bytes=A, steps=args.steps, warmup=args.warmup)

    def check(tag):
        torch.cuda.synchronize()
        assert bool((d_res == L).all()), tag + ": an open failed"
        v_pt, v_out = d_pt[: n * stride].view(n, stride)[:, :L], d_out[: n * stride].view(n, stride)[:, :L]
        assert torch.equal(v_pt, v_out), tag + ": round trip differs"
        d_out.zero_()
        d_res.zero_()

    # ChaCha20-Poly1305
    cks = ptls_hip.KeySet(eng, 32, nkeys, algo=ptls_hip.ALGO_CHACHA20POLY1305)
    cks.set(0, keys, ivs)

    def chacha_step(stream, ev):
        if ev:
            ev[0].record(stream)
        batch.chacha_seal(cks, d_pt, d_aad, d_ct, stream)
        if ev:
            ev[1].record(stream)
        batch.chacha_open(cks, d_ct, d_aad, d_out, d_res, stream)
        if ev:
            ev[2].record(stream)

    widths = [1, 4, 16, 64] if args.sweep_lanes else []
    for g in widths + [args.lanes]:
        batch.set_chacha_lanes(g)
        chacha_step(torch.cuda.current_stream(), None)
        check("chacha g=%d" % g)
        r = measure(chacha_step, args.steps, args.warmup, payload)
        r["lanes"] = batch.chacha_lanes
        if g == args.lanes:
            out["chacha20poly1305"] = r
        else:
            out.setdefault("chacha20poly1305_by_lanes", {})[str(g)] = r
    cks.close()

    # AES-128-GCM, same descriptors, same buffers, same clock
    aks = ptls_hip.KeySet(eng, 16, nkeys)
    aks.set(0, keys[: nkeys * 16], ivs)

    def aes_step(stream, ev):
        if ev:
            ev[0].record(stream)
        batch.seal(aks, d_pt, d_aad, d_ct, stream)
        if ev:
            ev[1].record(stream)
        batch.open(aks, d_ct, d_aad, d_out, d_res, stream)
        if ev:
            ev[2].record(stream)

    aes_step(torch.cuda.current_stream(), None)
    check("aes128gcm")
    r = measure(aes_step, args.steps, args.warmup, payload)
    r["lanes"] = batch.lanes
    out["aes128gcm"] = r
    aks.close()
    batch.close()
    out["chacha_over_aes"] = round(out["chacha20poly1305"]["seal_open_gibps"] / out["aes128gcm"]["seal_open_gibps"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", default="all", choices=["all"] + list(SHAPES))
    ap.add_argument("--lanes", type=int, default=0, choices=[0, 1, 4, 16, 64], help="ChaCha lanes per record (0 = automatic)")
    ap.add_argument("--sweep-lanes", action="store_true", help="also time the ChaCha kernel at every width")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a gfx950 device"
    eng = ptls_hip.Engine(0)
    for name in (list(SHAPES) if args.shape == "all" else [args.shape]):
        print(json.dumps(run_shape(eng, name, SHAPES[name], args)), flush=True)
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
