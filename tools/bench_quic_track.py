#!/usr/bin/env python3
"""The tracking of received packet numbers behind an open call (ptls_hip_quic_rx_track, include/ptls_hip.h 2k) beside the open
step and the key-phase commit (2j), in one process on one clock, over the same protected bytes.

  python tools/bench_quic_track.py [--steps K] [--warmup W] [--scale S] [--cipher aes128|chacha|all] [--workload ...]

Workloads (short-header packets of 1 350 payload bytes, tools/bench_quic_parse.py's SHORT; tools/bench_quic_keyphase.py's shapes):
  short   1 048 576 packets of 65 536 connections, 16 each
  onekey  262 144 packets of ONE connection, consecutive numbers: every atomic of the claim pass would go to one address were
          it not for the fold per lane and the reduction per wave

The entries are parsed once (ptls_hip_quic_rx_parse); every step starts from the same protected bytes, the same key-phase
table, empty packet-number spaces and the same expected-pn table.  Per step, on the host clock: open_step_ms
(rx_open_keyphase up to the end of its kernels), commit_call_ms and track_call_ms (each call ends in its own synchronisation).
With HIP events inside the calls (ptls_hip_quic_rx_timing, _keyphase_timing, _track_timing): commit_ms (the mark, flag, scan
and apply launches) and track_ms (the table reset, the claim, verdict, flag, scan and apply launches).  Medians of K steps
after W warm-ups.  Before the timing every verdict, the state table, the expected-pn table and the list of touched
connections are checked once, and once more for the replay of the same packets (all duplicates, nothing touched).  One JSON
line per workload and cipher.
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
from bench_quic_parse import CIPHERS, NCONN, SHORT, headers, median  # noqa: E402

WORKLOADS = {"short": dict(n=1 << 20, nconn=NCONN), "onekey": dict(n=1 << 18, nconn=1)}
STRIDE_BYTES = 1392
BASE = 1 << 32


def run(eng, name, cipher, args):
    w = WORKLOADS[name]
    n = max(1, w["n"] // args.scale)
    nconn = min(w["nconn"], n)
    algo, ksz = CIPHERS[cipher]
    rng = np.random.default_rng(9200)
    idx = np.arange(n, dtype=np.uint64)
    conn = (idx % np.uint64(nconn)).astype(np.uint32)
    cids = ((np.arange(nconn, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)).astype(">u8").view(np.uint8).reshape(nconn, 8)
    stride = nconn
    ks, hp = ptls_hip.KeySet(eng, ksz, 3 * stride, algo=algo), ptls_hip.KeySet(eng, ksz, nconn, algo=algo)
    ks.set(0, rng.integers(0, 256, 3 * stride * ksz, dtype=np.uint8).tobytes(), rng.integers(0, 256, 3 * stride * 12, dtype=np.uint8).tobytes())
    hp.set(0, rng.integers(0, 256, nconn * ksz, dtype=np.uint8).tobytes(), None)

    pn = idx + np.uint64(BASE)
    total = n * STRIDE_BYTES + 64
    d_pkt = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_pt = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
    h, pn_offset = headers(SHORT, cids[conn], pn)
    d_pkt[: n * STRIDE_BYTES].view(n, STRIDE_BYTES)[:, : h.shape[1]].copy_(torch.from_numpy(h).cuda())
    sealed = np.zeros(n, dtype=ptls_hip.QUIC_PACKET_DTYPE)
    sealed["pkt_off"] = idx * np.uint64(STRIDE_BYTES)
    sealed["data_off"] = sealed["pkt_off"] + np.uint64(pn_offset + 1)
    sealed["pn"], sealed["pkt_len"], sealed["hp_key"], sealed["key"] = pn, h.shape[1] + SHORT["payload"] + 16, conn, conn
    sealed["pn_offset"], sealed["pn_len"] = pn_offset, 4
    qs = ptls_hip.QuicBatch(eng, sealed, open=False)
    qs.seal(ks, hp, d_pt, d_pkt)
    torch.cuda.synchronize()
    qs.close()
    d_wire = d_pkt.clone()

    # the receiver: generation 0 everywhere, empty packet-number spaces, every expected packet number at the first one sent
    phase = np.zeros(nconn, dtype=ptls_hip.QUIC_KEYPHASE_DTYPE)
    phase["first_pn"] = np.uint64(1 << 33)
    spaces = np.zeros(3 * nconn, dtype=ptls_hip.QUIC_PNSPACE_DTYPE)
    expected = np.full(3 * nconn, BASE, dtype=np.uint64)
    # what the rule makes of it, with numpy: every packet is new; per connection the largest number and the numbers within 64 of it
    per = n // nconn
    assert per * nconn == n
    top = np.uint64(BASE) + np.arange(nconn, dtype=np.uint64) + np.uint64((per - 1) * nconn)
    window = np.zeros(nconn, dtype=np.uint64)
    for k in range(min(per, 64)):
        if k * nconn < 64:
            window |= np.uint64(1) << np.uint64(k * nconn)
    want_spaces = spaces.copy()
    want_spaces["next"][2::3], want_spaces["window"][2::3] = top + np.uint64(1), window
    want_expected = expected.copy()
    want_expected[2::3] = top + np.uint64(1)
    d_phase0, d_spaces0, d_expected0 = (torch.from_numpy(a.view(np.uint8)).cuda() for a in (phase, spaces, expected))
    d_phase, d_spaces, d_expected = d_phase0.clone(), d_spaces0.clone(), d_expected0.clone().view(torch.int64)

    cmap = ptls_hip.QuicCidMap(eng, nconn)
    cmap.set([c.tobytes() for c in cids], np.arange(nconn, dtype=np.uint32))
    dg = np.zeros(n, dtype=ptls_hip.QUIC_DATAGRAM_DTYPE)
    dg["off"], dg["len"] = idx * np.uint64(STRIDE_BYTES), sealed["pkt_len"][0]
    L = ptls_hip.lib()
    st = torch.cuda.current_stream()
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_pn = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_sel = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_gen = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_upd = torch.zeros(nconn, dtype=torch.int32, device="cuda")
    d_verdict = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_touched = torch.zeros(nconn, dtype=torch.int32, device="cuda")
    clock = time.perf_counter
    rx = ptls_hip.QuicRx(eng, n, n)
    assert rx.parse(dg, d_pkt, total, cidmap=cmap, short_cid_len=8, expected_pn=d_expected, expected_count=expected.size, stream=st) == n
    L.ptls_hip_quic_rx_timing(1, None, None)

    def fresh(state=True):
        d_pkt.copy_(d_wire)
        d_phase.copy_(d_phase0)
        if state:
            d_spaces.copy_(d_spaces0)
            d_expected.copy_(d_expected0.view(torch.int64))
        torch.cuda.synchronize()

    def step(state=True):
        fresh(state)
        t0 = clock()
        rep = rx.open_keyphase(ks, hp, d_phase, nconn, stride, d_gen, d_pkt, total, d_out, total, d_sel, d_res, d_pn, stream=st)
        torch.cuda.synchronize()
        t1 = clock()
        rx.keyphase_commit(d_phase, nconn, d_res, d_pn, d_gen, d_upd, stream=st)
        t2 = clock()
        n_touched = rx.track(d_spaces, nconn, d_sel, d_res, d_pn, d_verdict, d_touched, d_expected, expected.size, stream=st)
        t3 = clock()
        assert rep.n_selected == n
        commit_ms, track_ms = ctypes.c_float(), ctypes.c_float()
        L.ptls_hip_quic_rx_keyphase_timing(None, ctypes.byref(commit_ms))
        L.ptls_hip_quic_rx_track_timing(ctypes.byref(track_ms))
        return [(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, commit_ms.value, track_ms.value], n_touched

    # once: everything opened and new; then the same packets again from the state this left: all duplicates
    _, n_touched = step()
    assert (d_res.cpu().numpy().view(np.uint64) == SHORT["payload"]).all(), "open: results differ"
    assert np.array_equal(d_pn.cpu().numpy().view(np.uint64), pn), "open: packet numbers differ"
    assert (d_verdict.cpu().numpy() == ptls_hip.QUIC_PN_NEW).all(), "track: not every packet is new"
    assert np.array_equal(d_spaces.cpu().numpy().view(ptls_hip.QUIC_PNSPACE_DTYPE), want_spaces), "track: the state table differs"
    assert np.array_equal(d_expected.cpu().numpy().view(np.uint64), want_expected), "track: the expected-pn table differs"
    assert n_touched == nconn and np.array_equal(d_touched.cpu().numpy().view(np.uint32), np.arange(nconn, dtype=np.uint32)), "touched differs"
    _, n_touched = step(state=False)
    want_replay = np.where(top[conn] - pn < np.uint64(64), ptls_hip.QUIC_PN_DUPLICATE, ptls_hip.QUIC_PN_TOO_OLD)
    assert np.array_equal(d_verdict.cpu().numpy(), want_replay) and n_touched == 0, "replay: a packet was accepted twice"
    assert np.array_equal(d_spaces.cpu().numpy().view(ptls_hip.QUIC_PNSPACE_DTYPE), want_spaces), "replay: the state table changed"

    out = dict(workload=name, cipher=cipher, packets=n, connections=nconn, touched_connections=nconn, steps=args.steps, warmup=args.warmup)
    rows = [step()[0] for _ in range(args.warmup + args.steps)][args.warmup:]
    for k, f in enumerate(("open_step_ms", "commit_call_ms", "track_call_ms", "commit_ms", "track_ms")):
        out[f] = median([x[k] for x in rows])
    out["track_over_commit_call"] = round(out["track_call_ms"] / out["commit_call_ms"], 2) if out["commit_call_ms"] else None
    L.ptls_hip_quic_rx_timing(0, None, None)
    torch.cuda.synchronize()
    rx.close()
    cmap.close()
    ks.close()
    hp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1, help="divide the packet counts (a quick run)")
    ap.add_argument("--cipher", default="all", choices=["all", "aes128", "aes256", "chacha"])
    ap.add_argument("--workload", default="all", choices=["all"] + list(WORKLOADS))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a gfx950 device"
    eng = ptls_hip.Engine(0)
    for name in (list(WORKLOADS) if args.workload == "all" else [args.workload]):
        for cipher in (("aes128", "chacha") if args.cipher == "all" else (args.cipher,)):
            print(json.dumps(run(eng, name, cipher, args)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
