#!/usr/bin/env python3
"""The ACK frames written on the device (ptls_hip_quic_rx_ack, include/ptls_hip.h 2m) beside the host path the call replaces,
in one process on one clock, over the same state table and the same list.

  python tools/bench_quic_ack.py [--steps K] [--warmup W] [--scale S] [--loss P] [--workload ...]

Workloads (tools/bench_quic_track.py's two shapes, as rx_track's d_touched would list them):
  short   65 536 touched connections
  onekey  ONE touched connection: the floor of the call (four launches and one readback)

The state is the 1-RTT space of every connection: next somewhere above 1 000, the window with every packet but the largest
lost with probability P (default 0.05: a few ACK ranges per frame; 0: one range; 0.5: about sixteen).

Per step, on the host clock: ack_call_ms (the call ends in its own synchronisation), and host_path_ms for what it replaces:
the listed state entries gathered on the device and copied to the host, the frames and the requests built there with
vectorised numpy (no Python loop over connections: one pass per ACK range over all of them), both uploaded, up to the end of
the uploads; host_copy_ms, host_build_ms and host_upload_ms are its three parts.  With HIP events inside the call
(ptls_hip_quic_rx_timing, _ack_timing): ack_ms (the size, scan and write launches).  Medians of K steps after W warm-ups.
Before the timing the two paths' outputs are compared whole, once: the frame bytes, the requests, and the lengths and
offsets.  One JSON line per workload.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hsig-picotls_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ptls_hip  # noqa: E402
from bench_quic_parse import median  # noqa: E402

WORKLOADS = {"short": dict(nconn=1 << 16), "onekey": dict(nconn=1)}
ACK_MAX = ptls_hip.QUIC_ACK_MAX
U = np.uint64


def popcount(x):
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.uint32)


def zeros_below(x):
    """the clear bits below the lowest set bit (64 for 0)"""
    return popcount((x & (~x + U(1))) - U(1))


def down(x, by):
    """x >> by for by in 0 .. 64"""
    return np.where(by >= 64, U(0), x >> np.minimum(by, 63).astype(U))


def varint_columns(v):
    """the minimal varints of v as 8 right-aligned byte columns and their validity"""
    size = np.where(v < 64, 1, np.where(v < 16384, 2, np.where(v < 1 << 30, 4, 8))).astype(U)
    prefix = np.where(size == 1, 0, np.where(size == 2, 1, np.where(size == 4, 2, 3))).astype(U)
    x = v | prefix << (U(8) * size - U(2))
    k = np.arange(8, dtype=U)
    return ((x[:, None] >> (U(8) * (U(7) - k))[None, :]) & U(0xFF)).astype(np.uint8), k[None, :] >= (U(8) - size)[:, None]


def host_frames(states, conns, ack_delay, in_off, pkt_base, pkt_stride):
    """what a host does with the listed state entries (all of them acceptable): (frame bytes, lengths, offsets, requests)"""
    n = len(states)
    nxt, w = states["next"], states["window"]
    w = np.where(nxt >= 64, w, w & ((U(1) << np.minimum(nxt, 63).astype(U)) - U(1)))
    r = popcount(w & ~(w << U(1))) - 1
    tail = np.zeros((n, 64), dtype=np.uint8)
    tail[:, 0] = r
    run = zeros_below(~w)
    tail[:, 1] = run - 1
    rest = down(w, run)
    for i in range(int(r.max()) if n else 0):
        live = r > i
        gap = np.where(live, zeros_below(rest), 1)
        rest = down(rest, gap)
        run = np.where(live, zeros_below(~rest), 1)
        rest = down(rest, run)
        tail[:, 2 + 2 * i], tail[:, 3 + 2 * i] = gap - 1, run - 1
    big, big_ok = varint_columns(nxt - U(1))
    delay, delay_ok = varint_columns(np.full(n, ack_delay, dtype=U))
    rows = np.concatenate([np.full((n, 1), 2, np.uint8), big, delay, tail], axis=1)
    ok = np.concatenate([np.ones((n, 1), bool), big_ok, delay_ok, np.arange(64)[None, :] < (2 + 2 * r)[:, None]], axis=1)
    lens = ok.sum(axis=1).astype(np.uint32)
    offs = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint32)
    reqs = np.zeros(n, dtype=ptls_hip.QUIC_TXREQ_DTYPE)
    reqs["data_off"], reqs["pkt_off"] = U(in_off) + offs, U(pkt_base) + np.arange(n, dtype=U) * U(pkt_stride)
    reqs["conn"], reqs["len"] = conns, lens
    return rows[ok], lens, offs, reqs


def run(eng, name, args):
    nconn = max(1, WORKLOADS[name]["nconn"] // args.scale)
    rng = np.random.default_rng(9300)
    spaces = np.zeros(3 * nconn, dtype=ptls_hip.QUIC_PNSPACE_DTYPE)
    spaces["next"][2::3] = rng.integers(1000, 1 << 32, nconn, dtype=np.uint64)
    kept = np.packbits(rng.random((nconn, 64)) >= args.loss, axis=1, bitorder="little").view(np.uint64).reshape(nconn)
    spaces["window"][2::3] = kept | U(1)
    conns = np.arange(nconn, dtype=np.uint32)  # rx_track's d_touched: ascending
    n, delay, in_off, base, stride = nconn, 25, 4096, 0, 128
    d_spaces = torch.from_numpy(spaces.view(np.uint8)).cuda()
    d_list = torch.from_numpy(conns.view(np.int32)).cuda()
    d_frames = torch.zeros(ACK_MAX * n, dtype=torch.uint8, device="cuda")
    d_status, d_off, d_len = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
    d_reqs = torch.zeros(n * ptls_hip.QUIC_TXREQ_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_frames2, d_reqs2 = torch.zeros_like(d_frames), torch.zeros_like(d_reqs)
    places = (3 * d_list.long() + 2)
    L = ptls_hip.lib()
    st = torch.cuda.current_stream()
    clock = time.perf_counter
    rx = ptls_hip.QuicRx(eng, 0, 1)
    L.ptls_hip_quic_rx_timing(1, None, None)

    def device_step():
        torch.cuda.synchronize()
        t0 = clock()
        rep = rx.ack(d_spaces, nconn, 2, d_list, n, d_frames, ACK_MAX * n, d_status, d_off, d_len, d_reqs, ack_delay=delay, in_off=in_off,
                     pkt_base=base, pkt_stride=stride, stream=st)
        t1 = clock()
        ms = ctypes.c_float()
        L.ptls_hip_quic_rx_ack_timing(ctypes.byref(ms))
        return rep, [(t1 - t0) * 1e3, ms.value]

    def host_step():
        torch.cuda.synchronize()
        t0 = clock()
        listed = d_spaces.view(-1, 16)[places].cpu().numpy().view(ptls_hip.QUIC_PNSPACE_DTYPE).reshape(n)
        t1 = clock()
        frames, lens, offs, reqs = host_frames(listed, conns, delay, in_off, base, stride)
        t2 = clock()
        d_frames2[:frames.size].copy_(torch.from_numpy(frames), non_blocking=True)
        d_reqs2.copy_(torch.from_numpy(reqs.view(np.uint8)), non_blocking=True)
        torch.cuda.synchronize()
        t3 = clock()
        return (frames, lens, offs, reqs), [(t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3]

    # once: the two paths' outputs, whole
    rep, _ = device_step()
    (frames, lens, offs, reqs), _ = host_step()
    assert rep.n_frames == n and rep.bytes == frames.size, "the sums differ"
    assert (d_status.cpu().numpy() == ptls_hip.QUIC_ACK_OK).all(), "a listed entry got no frame"
    assert np.array_equal(d_len.cpu().numpy().view(np.uint32), lens) and np.array_equal(d_off.cpu().numpy().view(np.uint32), offs), \
        "lengths or offsets differ"
    assert np.array_equal(d_frames.cpu().numpy()[:frames.size], frames), "the frame bytes differ"
    assert np.array_equal(d_frames2.cpu().numpy()[:frames.size], frames) and torch.equal(d_reqs, d_reqs2), "the requests differ"

    out = dict(workload=name, connections=nconn, loss=args.loss, frames=int(rep.n_frames), frame_bytes=int(rep.bytes),
               mean_frame_bytes=round(rep.bytes / n, 2), max_frame_bytes=int(lens.max()), steps=args.steps, warmup=args.warmup)
    dev_rows = [device_step()[1] for _ in range(args.warmup + args.steps)][args.warmup:]
    host_rows = [host_step()[1] for _ in range(args.warmup + args.steps)][args.warmup:]
    for k, f in enumerate(("ack_call_ms", "ack_ms")):
        out[f] = median([x[k] for x in dev_rows])
    for k, f in enumerate(("host_path_ms", "host_copy_ms", "host_build_ms", "host_upload_ms")):
        out[f] = median([x[k] for x in host_rows])
    out["host_over_call"] = round(out["host_path_ms"] / out["ack_call_ms"], 2) if out["ack_call_ms"] else None
    L.ptls_hip_quic_rx_timing(0, None, None)
    torch.cuda.synchronize()
    rx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide the connection count (a quick run)")
    ap.add_argument("--loss", type=float, default=0.05, help="the probability that a packet of the window is missing")
    ap.add_argument("--workload", default="all", choices=["all"] + list(WORKLOADS))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a gfx950 device"
    eng = ptls_hip.Engine(0)
    for name in (list(WORKLOADS) if args.workload == "all" else [args.workload]):
        print(json.dumps(run(eng, name, args)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
