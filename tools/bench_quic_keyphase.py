#!/usr/bin/env python3
"""The open step of the receive object with the key taken from the descriptor (ptls_hip_quic_rx_open, include/ptls_hip.h 2i)
against the key chosen by Key Phase bit and the commit of key updates (ptls_hip_quic_rx_open_keyphase +
ptls_hip_quic_rx_keyphase_commit, 2j), in one process on one clock, over the same protected bytes.

  python tools/bench_quic_keyphase.py [--steps K] [--warmup W] [--scale S] [--cipher aes128|chacha|all] [--workload ...]

Workloads (short-header packets of 1 350 payload bytes, tools/bench_quic_parse.py's SHORT):
  short   1 048 576 packets of 65 536 connections, every one of generation 0: the keys sit in bank 0 of a keyset of three
          banks, so both calls open every packet
  mix     the same, with every third connection mid-update: the second half of its packets carries the other Key Phase bit and
          is sealed under generation 1 (bank 1).  rx_open, which takes `key` as it is, fails exactly those; open_keyphase opens
          all, and the commit advances exactly those connections
  onekey  262 144 packets of ONE connection: rx_open plans AES on the host for the batch kernel; open_keyphase always takes the
          wave-per-record kernel

The entries are parsed once (ptls_hip_quic_rx_parse); every step starts from the same protected bytes and the same state
table.  Per step, alternating the two paths, on the host clock up to the end of the kernels: plain_call_ms + plain_tail_ms =
plain_step_ms; kp_call_ms + kp_tail_ms + commit_call_ms (the commit ends in its own synchronisation) = kp_step_ms.  With HIP
events inside the calls (ptls_hip_quic_rx_timing, ptls_hip_quic_rx_keyphase_timing): select_ms, sort_ms, header_ms
(quic_unprotect_phase_kernel) and commit_ms (the mark, flag, scan and apply launches).  Medians of K steps after W warm-ups.
Before the timing every result, packet number, generation and plaintext byte of the key-phase path, the state table after
the commit and the list of updated connections are checked once.  One JSON line per workload and cipher.
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

WORKLOADS = {"short": dict(n=1 << 20, nconn=NCONN, updating=0), "mix": dict(n=1 << 20, nconn=NCONN, updating=3),
             "onekey": dict(n=1 << 18, nconn=1, updating=0)}
STRIDE_BYTES = 1392
U64 = (1 << 64) - 1


def run(eng, name, cipher, args):
    w = WORKLOADS[name]
    n = max(1, w["n"] // args.scale)
    nconn = min(w["nconn"], n)
    algo, ksz = CIPHERS[cipher]
    rng = np.random.default_rng(9100)
    idx = np.arange(n, dtype=np.uint64)
    conn = (idx % np.uint64(nconn)).astype(np.uint32)
    cids = ((np.arange(nconn, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)).astype(">u8").view(np.uint8).reshape(nconn, 8)
    stride = nconn  # the bank stride: generation g of connection c in slot c + stride * (g % 3)
    ks, hp = ptls_hip.KeySet(eng, ksz, 3 * stride, algo=algo), ptls_hip.KeySet(eng, ksz, nconn, algo=algo)
    ks.set(0, rng.integers(0, 256, 3 * stride * ksz, dtype=np.uint8).tobytes(), rng.integers(0, 256, 3 * stride * 12, dtype=np.uint8).tobytes())
    hp.set(0, rng.integers(0, 256, nconn * ksz, dtype=np.uint8).tobytes(), None)

    # the sender: generation 1 for the second half of the packets of every `updating`-th connection
    pn = idx + np.uint64(1 << 32)
    first_new = np.uint64(1 << 32) + np.uint64(n // 2)
    updating = (conn % np.uint32(w["updating"]) == 1) if w["updating"] else np.zeros(n, bool)
    gen1 = updating & (pn >= first_new)
    total = n * STRIDE_BYTES + 64
    d_pkt = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_pt = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
    h, pn_offset = headers(SHORT, cids[conn], pn)
    h[gen1, 0] |= 0x04
    d_pkt[: n * STRIDE_BYTES].view(n, STRIDE_BYTES)[:, : h.shape[1]].copy_(torch.from_numpy(h).cuda())
    sealed = np.zeros(n, dtype=ptls_hip.QUIC_PACKET_DTYPE)
    sealed["pkt_off"] = idx * np.uint64(STRIDE_BYTES)
    sealed["data_off"] = sealed["pkt_off"] + np.uint64(pn_offset + 1)
    sealed["pn"], sealed["pkt_len"], sealed["hp_key"] = pn, h.shape[1] + SHORT["payload"] + 16, conn
    sealed["key"] = conn + np.uint32(stride) * gen1.astype(np.uint32)
    sealed["pn_offset"], sealed["pn_len"] = pn_offset, 4
    qs = ptls_hip.QuicBatch(eng, sealed, open=False)
    qs.seal(ks, hp, d_pt, d_pkt)
    torch.cuda.synchronize()
    qs.close()
    d_wire = d_pkt.clone()
    want_len = np.full(n, SHORT["payload"], np.uint64)

    # the receiver: every connection at generation 0, its lowest packet number so far above every one of this call's (the
    # commit has a minimum to find for each connection)
    table = np.zeros(nconn, dtype=ptls_hip.QUIC_KEYPHASE_DTYPE)
    table["first_pn"] = np.uint64(1 << 33)
    want_gen = gen1.astype(np.uint32)
    want_upd = np.unique(conn[gen1])
    want_table = table.copy()
    lowest_cur = np.full(nconn, U64, np.uint64)
    np.minimum.at(lowest_cur, conn[~gen1], pn[~gen1])
    want_table["first_pn"] = np.minimum(table["first_pn"], lowest_cur)
    assert (want_table["first_pn"] == np.uint64(1 << 32) + np.arange(nconn, dtype=np.uint64)).all()
    want_table["gen"][want_upd] = 1
    for c in want_upd[:64]:  # (spot check of the rule in plain Python; the whole table below with numpy)
        assert int(pn[(conn == c) & gen1].min()) >= int(first_new)
    if len(want_upd):
        lowest = np.full(nconn, U64, np.uint64)
        np.minimum.at(lowest, conn[gen1], pn[gen1])
        want_table["first_pn"][want_upd] = lowest[want_upd]
    d_table0 = torch.from_numpy(table.view(np.uint8)).cuda()
    d_table = d_table0.clone()

    cmap = ptls_hip.QuicCidMap(eng, nconn)
    cmap.set([c.tobytes() for c in cids], np.arange(nconn, dtype=np.uint32))
    expected = np.full((nconn, 3), 1 << 32, dtype=np.uint64)
    d_expected = torch.from_numpy(expected.view(np.int64).reshape(-1)).cuda()
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
    clock = time.perf_counter
    rx = ptls_hip.QuicRx(eng, n, n)
    assert rx.parse(dg, d_pkt, total, cidmap=cmap, short_cid_len=8, expected_pn=d_expected, expected_count=expected.size, stream=st) == n
    L.ptls_hip_quic_rx_timing(1, None, None)

    def fresh():
        d_pkt.copy_(d_wire)
        d_table.copy_(d_table0)
        torch.cuda.synchronize()

    def timing():
        v = [ctypes.c_float() for _ in range(4)]
        L.ptls_hip_quic_rx_timing(1, ctypes.byref(v[0]), ctypes.byref(v[1]))
        L.ptls_hip_quic_rx_keyphase_timing(ctypes.byref(v[2]), ctypes.byref(v[3]))
        return [x.value for x in v]

    def plain_step():
        fresh()
        t0 = clock()
        rep = rx.open(ks, hp, d_pkt, total, d_out, total, d_sel, d_res, d_pn, stream=st)
        t1 = clock()
        torch.cuda.synchronize()
        t2 = clock()
        assert rep.n_selected == n
        return [(b - a) * 1e3 for a, b in ((t0, t1), (t1, t2), (t0, t2))], rep

    def kp_step():
        fresh()
        t0 = clock()
        rep = rx.open_keyphase(ks, hp, d_table, nconn, stride, d_gen, d_pkt, total, d_out, total, d_sel, d_res, d_pn, stream=st)
        t1 = clock()
        torch.cuda.synchronize()
        t2 = clock()
        n_upd = rx.keyphase_commit(d_table, nconn, d_res, d_pn, d_gen, d_upd, stream=st)
        t3 = clock()
        assert rep.n_selected == n
        return [(b - a) * 1e3 for a, b in ((t0, t1), (t1, t2), (t2, t3), (t0, t3))] + timing(), rep, n_upd

    # once: the plain path fails exactly the next-generation packets; the key-phase path against what was sealed
    _, rep0 = plain_step()
    res = d_res.cpu().numpy().view(np.uint64)
    assert np.array_equal(res == U64, gen1) and np.array_equal(res[~gen1], want_len[~gen1]), "rx_open: unexpected results"
    d_out.zero_()
    d_res.zero_()
    d_pn.zero_()
    _, rep, n_upd = kp_step()
    assert np.array_equal(d_res.cpu().numpy().view(np.uint64), want_len), "open_keyphase: results differ"
    assert np.array_equal(d_pn.cpu().numpy().view(np.uint64), pn), "open_keyphase: packet numbers differ"
    assert np.array_equal(d_gen.cpu().numpy().view(np.uint32), want_gen), "open_keyphase: generations differ"
    assert np.array_equal(d_sel.cpu().numpy().view(np.uint32), np.arange(n, dtype=np.uint32)), "open_keyphase: selection differs"
    o = int(sealed["data_off"][0])
    assert torch.equal(d_out[: n * STRIDE_BYTES].view(n, STRIDE_BYTES)[:, o: o + SHORT["payload"]],
                       d_pt[: n * STRIDE_BYTES].view(n, STRIDE_BYTES)[:, o: o + SHORT["payload"]]), "plaintext differs"
    assert n_upd == len(want_upd) and np.array_equal(d_upd.cpu().numpy().view(np.uint32)[:n_upd], want_upd), "updated connections differ"
    assert np.array_equal(d_table.cpu().numpy().view(ptls_hip.QUIC_KEYPHASE_DTYPE), want_table), "the state table differs"

    out = dict(workload=name, cipher=cipher, packets=n, connections=nconn, next_generation_packets=int(gen1.sum()),
               updated_connections=int(n_upd), steps=args.steps, warmup=args.warmup,
               plain_planned_on_device=int(rep0.planned_on_device), plain_lanes=int(rep0.lanes),
               kp_planned_on_device=int(rep.planned_on_device), kp_lanes=int(rep.lanes))
    plain, kp = [], []
    for _ in range(args.warmup + args.steps):  # alternating, so that both see the same machine
        plain.append(plain_step()[0])
        kp.append(kp_step()[0])
    plain, kp = plain[args.warmup:], kp[args.warmup:]
    for k, f in enumerate(("plain_call_ms", "plain_tail_ms", "plain_step_ms")):
        out[f] = median([x[k] for x in plain])
    for k, f in enumerate(("kp_call_ms", "kp_tail_ms", "commit_call_ms", "kp_step_ms", "select_ms", "sort_ms", "header_ms", "commit_ms")):
        out[f] = median([x[k] for x in kp])
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
