#!/usr/bin/env python3
"""The receive step for datagrams resident on the device, the three existing calls against the receive object
(include/ptls_hip.h 2i), in one process on one clock.

  python tools/bench_quic_rx.py [--steps K] [--warmup W] [--scale S] [--cipher aes128|chacha|all] [--workload ...]

Workloads: `short` and `coalesced` of tools/bench_quic_parse.py (1 048 576 short-header packets; 262 144 datagrams of an
Initial, a Handshake and a 1-RTT packet: 786 432 packets; 65 536 connections each), and `onekey`: 262 144 short-header packets
of ONE connection, which the planner gives to the AES batch kernel, so the receive object plans it on the host.

Per workload and cipher, medians of K steps after W warm-up steps, every step from the same protected bytes:
  old   ptls_hip_quic_parse_datagrams (pageable host arrays) + ptls_hip_quic_batch_new(open) + ptls_hip_quic_open_batch, up to
        the end of the open kernel, on the host clock: parse_ms, plan_ms, open_ms (launch to completion) and their sum
        old_step_ms; batch_free_ms beside it (not in the sum)
  rx    ptls_hip_quic_rx_parse + ptls_hip_quic_rx_open, up to the end of the open kernel, on the host clock: rx_parse_ms,
        rx_open_call_ms (the call: select, the readback, the launches), rx_tail_ms (the wait for the kernels in flight) and
        their sum rx_step_ms; inside rx_open with HIP events (ptls_hip_quic_rx_timing) select_ms (select, scans, compact, sums)
        and sort_ms (the radix passes; 0 where there is no device sort)
Before the timing every selection index, result, packet number and plaintext byte of the rx path is checked once, and the
results of both paths against each other.  One JSON line per workload and cipher.
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
from bench_quic_parse import CIPHERS, NCONN, SHORT, WORKLOADS as PARSE_WORKLOADS, headers, median  # noqa: E402

WORKLOADS = dict(PARSE_WORKLOADS, onekey=dict(n=1 << 18, stride=1392, packets=[SHORT], nconn=1))


def run(eng, name, cipher, args):
    w = WORKLOADS[name]
    n, stride = max(1, w["n"] // args.scale), w["stride"]
    nconn = min(w.get("nconn", NCONN), n)
    algo, ksz = CIPHERS[cipher]
    rng = np.random.default_rng(9000)
    idx = np.arange(n, dtype=np.uint64)
    conn = (idx % np.uint64(nconn)).astype(np.uint32)
    cids = ((np.arange(nconn, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)).astype(">u8").view(np.uint8).reshape(nconn, 8)
    ks, hp = ptls_hip.KeySet(eng, ksz, nconn, algo=algo), ptls_hip.KeySet(eng, ksz, nconn, algo=algo)
    ks.set(0, rng.integers(0, 256, nconn * ksz, dtype=np.uint8).tobytes(), rng.integers(0, 256, nconn * 12, dtype=np.uint8).tobytes())
    hp.set(0, rng.integers(0, 256, nconn * ksz, dtype=np.uint8).tobytes(), None)

    total = n * stride + 64
    d_pkt = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_pt = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
    seal, off = [], 0
    for p in w["packets"]:
        pn = idx + np.uint64(1 << 32) + np.uint64(p["space"] << 40)
        h, pn_offset = headers(p, cids[conn], pn)
        d_pkt[: n * stride].view(n, stride)[:, off: off + h.shape[1]].copy_(torch.from_numpy(h).cuda())
        pk = np.zeros(n, dtype=ptls_hip.QUIC_PACKET_DTYPE)
        pk["pkt_off"] = idx * np.uint64(stride) + np.uint64(off)
        pk["data_off"] = pk["pkt_off"] + np.uint64(pn_offset + 1)
        pk["pn"], pk["pkt_len"], pk["key"], pk["hp_key"] = pn, h.shape[1] + p["payload"] + 16, conn, conn
        pk["pn_offset"], pk["pn_len"] = pn_offset, 4
        seal.append(pk)
        off += int(pk["pkt_len"][0])
    dgram_len = off
    sealed = np.stack(seal, axis=1).reshape(-1)
    qs = ptls_hip.QuicBatch(eng, sealed, open=False)
    qs.seal(ks, hp, d_pt, d_pkt)
    torch.cuda.synchronize()
    qs.close()
    d_wire = d_pkt.clone()
    want_len = (sealed["pkt_len"] - sealed["pn_offset"] - 4 - 16).astype(np.uint64)

    cmap = ptls_hip.QuicCidMap(eng, nconn)
    cmap.set([c.tobytes() for c in cids], np.arange(nconn, dtype=np.uint32))
    expected = np.zeros((nconn, 3), dtype=np.uint64)
    for s in range(3):
        expected[:, s] = np.uint64(1 << 32) + np.uint64(s << 40)
    d_expected = torch.from_numpy(expected.view(np.int64).reshape(-1)).cuda()
    dg = np.zeros(n, dtype=ptls_hip.QUIC_DATAGRAM_DTYPE)
    dg["off"], dg["len"] = idx * np.uint64(stride), dgram_len
    params = ptls_hip.QuicParseParams(8, 16, 1, 0, d_expected.data_ptr(), expected.size)
    npk = len(sealed)
    L = ptls_hip.lib()
    st = torch.cuda.current_stream()
    stream = st.cuda_stream
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(npk, dtype=torch.int64, device="cuda")
    d_pn = torch.zeros(npk, dtype=torch.int64, device="cuda")
    d_sel = torch.zeros(npk, dtype=torch.int32, device="cuda")
    pkts, info = np.zeros(npk, dtype=ptls_hip.QUIC_PACKET_DTYPE), np.zeros(npk, dtype=ptls_hip.QUIC_PKTINFO_DTYPE)
    clock = time.perf_counter

    def fresh():
        d_pkt.copy_(d_wire)
        torch.cuda.synchronize()

    def old_step():
        fresh()
        got = ctypes.c_size_t(0)
        t0 = clock()
        rc = L.ptls_hip_quic_parse_datagrams(eng.ptr, ctypes.addressof(params), cmap.ptr, dg.ctypes.data, n, d_pkt.data_ptr(), total,
                                             pkts.ctypes.data, info.ctypes.data, npk, ctypes.byref(got), stream)
        t1 = clock()
        assert rc == 0 and got.value == npk, ptls_hip.last_error()
        q = ptls_hip.QuicBatch(eng, pkts, open=True)
        t2 = clock()
        q.open(ks, hp, d_pkt, d_out, d_res, d_pn, st)
        torch.cuda.synchronize()
        t3 = clock()
        lanes = q.records().chacha_lanes if cipher == "chacha" else q.records().lanes
        q.close()
        t4 = clock()
        return [(b - a) * 1e3 for a, b in ((t0, t1), (t1, t2), (t2, t3), (t0, t3), (t3, t4))], lanes

    rx = ptls_hip.QuicRx(eng, n, npk)
    L.ptls_hip_quic_rx_timing(1, None, None)

    def rx_step():
        fresh()
        t0 = clock()
        got = rx.parse(dg, d_pkt, total, cidmap=cmap, short_cid_len=8, expected_pn=d_expected, expected_count=expected.size, stream=st)
        t1 = clock()
        rep = rx.open(ks, hp, d_pkt, total, d_out, total, d_sel, d_res, d_pn, stream=st)
        t2 = clock()
        torch.cuda.synchronize()
        t3 = clock()
        assert got == npk and rep.n_selected == npk
        a, b = ctypes.c_float(), ctypes.c_float()
        L.ptls_hip_quic_rx_timing(1, ctypes.byref(a), ctypes.byref(b))
        return [(y - x) * 1e3 for x, y in ((t0, t1), (t1, t2), (t2, t3), (t0, t3))] + [a.value, b.value], rep

    def outputs():
        return d_res.cpu().numpy().view(np.uint64).copy(), d_pn.cpu().numpy().view(np.uint64).copy()

    # once: the old path's outputs, then the rx path's against them and against what was sealed
    d_out.zero_()
    old_step()
    old_out = outputs()
    assert np.array_equal(old_out[0], want_len) and np.array_equal(old_out[1], sealed["pn"]), "the existing path failed"
    d_out.zero_()
    d_res.zero_()
    d_pn.zero_()
    _, rep = rx_step()
    new_out = outputs()
    assert np.array_equal(new_out[0], old_out[0]) and np.array_equal(new_out[1], old_out[1]), "rx results differ"
    assert np.array_equal(d_sel.cpu().numpy().view(np.uint32), np.arange(npk, dtype=np.uint32)), "rx selection differs"
    for pk, p in zip(seal, w["packets"]):
        o = int(pk["data_off"][0])
        a = d_out[: n * stride].view(n, stride)[:, o: o + p["payload"]]
        assert torch.equal(a, d_pt[: n * stride].view(n, stride)[:, o: o + p["payload"]]), "plaintext differs"

    out = dict(workload=name, cipher=cipher, datagrams=n, packets=npk, cids=nconn, steps=args.steps, warmup=args.warmup,
               planned_on_device=int(rep.planned_on_device), rx_lanes=int(rep.lanes))
    t = [old_step() for _ in range(args.warmup + args.steps)][args.warmup:]
    for k, f in enumerate(("parse_ms", "plan_ms", "open_ms", "old_step_ms", "batch_free_ms")):
        out[f] = median([x[0][k] for x in t])
    out["old_lanes"] = t[0][1]
    t = [rx_step()[0] for _ in range(args.warmup + args.steps)][args.warmup:]
    for k, f in enumerate(("rx_parse_ms", "rx_open_call_ms", "rx_tail_ms", "rx_step_ms", "select_ms", "sort_ms")):
        out[f] = median([x[k] for x in t])
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
    ap.add_argument("--scale", type=int, default=1, help="divide the datagram counts (a quick run)")
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
