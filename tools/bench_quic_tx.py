#!/usr/bin/env python3
"""The send object (include/ptls_hip.h 2l) beside the path it replaces, in one process.

  tx        ptls_hip_quic_tx_seal over requests and a state table that are already in device memory (host clock around the
            call and a synchronisation), and the HIP-event times of its launches in front of the record kernel and of its sort
  replaced  what a 2e sender does per batch: the header bytes written on the host (numpy), uploaded and placed in the packet
            buffer, the 40-byte descriptors filled and uploaded, ptls_hip_quic_batch_new (which plans on the host), and
            ptls_hip_quic_seal_batch

Shapes (§10.5's): short = 1 048 576 packets of 1 350 payload bytes over 65 536 connections, 16 in a row per connection;
onekey = 262 144 on one connection.  Medians of --steps steps after --warmup warm-ups; every step starts from the same state
table.  The two paths' packet buffers are compared whole once before the timing."""
import argparse
import hashlib
import json
import statistics
import sys
import time
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hsig-picotls_amd"))
import ptls_hip  # noqa: E402

ALGOS = {"aes128": (ptls_hip.ALGO_AESGCM, 16), "chacha": (ptls_hip.ALGO_CHACHA20POLY1305, 32)}
PAYLOAD, DCID = 1350, 8


def material(tag, n):
    out, i = bytearray(), 0
    while len(out) < n:
        out += hashlib.sha256(b"%s/%d" % (tag.encode(), i)).digest()
        i += 1
    return bytes(out[:n])


def shape(name, scale):
    if name == "short":
        return max(1, 65536 // scale), 16
    return 1, max(1, 262144 // scale)


def run(engine, algo, name, scale, steps, warmup):
    kind, ksz = ALGOS[algo]
    conns, per = shape(name, scale)
    n = conns * per
    stride = conns
    ks, hp = ptls_hip.KeySet(engine, ksz, 3 * stride, algo=kind), ptls_hip.KeySet(engine, ksz, conns, algo=kind)
    ks.set(0, material("k", 3 * stride * ksz), material("i", 3 * stride * 12))
    hp.set(0, material("h", conns * ksz), None)
    # the state: every connection has sent 1 000 packets, the peer has acknowledged all but 100; three-byte numbers throughout
    # (params.pn_len = 3: the longest run's last number needs them, and every packet then has one length)
    table = np.zeros(conns, dtype=ptls_hip.QUIC_TXCONN_DTYPE)
    table["next_pn"], table["largest_acked"], table["gen"] = 1000, 899, np.arange(conns) % 3
    table["dcid_len"] = DCID
    table["dcid"][:, :DCID] = np.frombuffer(material("d", conns * DCID), np.uint8).reshape(conns, DCID)
    pn_len, hdr_len = 3, 1 + DCID + 3
    pkt_len = hdr_len + PAYLOAD + 16
    area = (pkt_len + 15) & ~15
    reqs = np.zeros(n, dtype=ptls_hip.QUIC_TXREQ_DTYPE)
    idx = np.arange(n, dtype=np.uint64)
    reqs["conn"], reqs["len"] = (idx // per).astype(np.uint32), PAYLOAD
    reqs["data_off"], reqs["pkt_off"] = idx * np.uint64(1360), idx * np.uint64(area)
    in_len, buf_len = n * 1360, n * area
    d_in = torch.randint(0, 256, (in_len,), dtype=torch.uint8, device="cuda")
    d_pkt, d_pkt2 = torch.zeros(buf_len, dtype=torch.uint8, device="cuda"), torch.zeros(buf_len, dtype=torch.uint8, device="cuda")
    d_table0 = torch.from_numpy(table.view(np.uint8)).cuda()
    d_table = d_table0.clone()
    d_reqs = torch.from_numpy(reqs.view(np.uint8)).cuda()
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_pn = torch.zeros(n, dtype=torch.int64, device="cuda")
    tx = ptls_hip.QuicTx(engine, n)
    L = ptls_hip.lib()
    import ctypes

    def tx_step():
        d_table.copy_(d_table0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = tx.seal(ks, hp, d_table, conns, stride, d_reqs, n, d_in, in_len, d_pkt, buf_len, d_status, d_pn, d_len, pn_len=pn_len)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        front, sort = ctypes.c_float(0), ctypes.c_float(0)
        L.ptls_hip_quic_tx_timing(1, ctypes.byref(front), ctypes.byref(sort))
        return ms, front.value, sort.value, rep

    pos = torch.from_numpy((reqs["pkt_off"].astype(np.int64)[:, None] + np.arange(hdr_len, dtype=np.int64)[None, :]).reshape(-1)).cuda()

    def replaced_step():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        # the host's part: numbers, lengths, header bytes, descriptors
        conn = reqs["conn"]
        pn = table["next_pn"][conn] + (idx % np.uint64(per))
        gen = table["gen"][conn]
        hdr = np.empty((n, hdr_len), np.uint8)
        hdr[:, 0] = 0x40 | ((gen & 1) << 2).astype(np.uint8) | (pn_len - 1)
        hdr[:, 1:1 + DCID] = table["dcid"][conn, :DCID]
        hdr[:, 1 + DCID] = (pn >> np.uint64(16)).astype(np.uint8)
        hdr[:, 2 + DCID] = (pn >> np.uint64(8)).astype(np.uint8)
        hdr[:, 3 + DCID] = pn.astype(np.uint8)
        desc = np.zeros(n, dtype=ptls_hip.QUIC_PACKET_DTYPE)
        desc["pkt_off"], desc["data_off"], desc["pn"], desc["pkt_len"] = reqs["pkt_off"], reqs["data_off"], pn, pkt_len
        desc["key"], desc["hp_key"] = conn + np.uint32(stride) * (gen % 3).astype(np.uint32), conn
        desc["pn_offset"], desc["pn_len"] = 1 + DCID, pn_len
        t_host = time.perf_counter()
        d_pkt2[pos] = torch.from_numpy(hdr.reshape(-1)).cuda()
        q = ptls_hip.QuicBatch(engine, desc, open=False)
        t_new = time.perf_counter()
        q.seal(ks, hp, d_in, d_pkt2)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lanes = q.records().chacha_lanes if algo == "chacha" else q.records().lanes
        q.close()
        return (t1 - t0) * 1e3, (t_host - t0) * 1e3, (t_new - t_host) * 1e3, (t1 - t_new) * 1e3, lanes

    L.ptls_hip_quic_tx_timing(1, None, None)
    _, _, _, rep = tx_step()
    lanes = replaced_step()[4]
    torch.cuda.synchronize()
    assert rep.n_sent == n and rep.bytes == n * pkt_len and bool((d_status == 0).all()) and bool((d_len == pkt_len).all())
    assert torch.equal(d_pkt, d_pkt2), "the two paths' packet buffers differ"
    want_next = torch.from_numpy((table["next_pn"] + np.uint64(per)).astype(np.int64)).cuda()
    got_next = d_table.view(torch.int64).view(conns, 6)[:, 0]
    assert torch.equal(got_next, want_next)
    a = [tx_step()[:3] for _ in range(warmup + steps)][warmup:]
    b = [replaced_step()[:4] for _ in range(warmup + steps)][warmup:]
    med = lambda rows, k: round(statistics.median(r[k] for r in rows), 3)  # noqa: E731
    out = {"shape": name, "algo": algo, "packets": n, "connections": conns, "payload": PAYLOAD, "steps": steps, "warmup": warmup,
           "tx_call_ms": med(a, 0), "tx_front_events_ms": med(a, 1), "tx_sort_events_ms": med(a, 2), "tx_lanes": rep.lanes,
           "replaced_ms": med(b, 0), "replaced_host_fill_ms": med(b, 1), "replaced_upload_and_batch_new_ms": med(b, 2),
           "replaced_seal_batch_ms": med(b, 3), "replaced_lanes": lanes, "outputs_equal": True}
    tx.close()
    ks.close()
    hp.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="short,onekey")
    ap.add_argument("--algos", default="aes128,chacha")
    ap.add_argument("--scale", type=int, default=1, help="divide the shapes' sizes (for a quick look)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    engine = ptls_hip.Engine(0)
    for name in args.shapes.split(","):
        for algo in args.algos.split(","):
            print(json.dumps(run(engine, algo, name, args.scale, args.steps, args.warmup)), flush=True)
    engine.close()


if __name__ == "__main__":
    main()
