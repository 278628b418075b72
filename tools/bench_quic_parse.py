#!/usr/bin/env python3
"""QUIC datagrams parsed on the device (ptls_hip_quic_parse_datagrams) next to the open call they feed and next to the same
walk on one host core, in one process on one clock.

  python tools/bench_quic_parse.py [--steps K] [--warmup W] [--scale S] [--cipher aes128|aes256|chacha]

Workloads (S = 1; --scale divides the datagram counts):
  short      1 048 576 datagrams of one short-header packet each: 1 350 payload bytes, an 8-byte DCID, 4 packet-number bytes,
             1 379 bytes at a 1 392-byte stride, over 65 536 connection IDs (datagram i: connection i % 65 536)
  coalesced  262 144 datagrams of an Initial (250 payload bytes), a Handshake (400) and a 1-RTT packet (600) of one connection
             coalesced, 1 354 bytes at a 1 360-byte stride, over 65 536 connection IDs: 786 432 packets

The packets are sealed on the device first (QuicBatch.seal), so what is parsed opens.  Per workload, medians of K steps after W
warm-up steps:
  parse      the whole synchronous call on the host clock (call_ms), and inside it with HIP events (ptls_hip_quic_parse_timing)
             the kernels (upload of the datagram array, count, scans, write: kernels_ms) and the copy of the entries back
             (d2h_ms), into pageable and into pinned host arrays
  plan       ptls_hip_quic_batch_new(open) over the parsed descriptors, host clock (the planning the host still does)
  open       QuicBatch.open over them, HIP events (open_ms); the record kernel alone over descriptors the host already knows,
             headers unprotected (record_ms); their difference is quic_unprotect_kernel (unprotect_ms)
  host       the same walk and map lookup (csrc/quic_parse.h, tools/quic_parse_host/quic_parse_host.cpp, g++ -O2) on one core
             over the same bytes in host memory (host_walk_ms)
Every parsed entry is checked against the descriptors the packets were sealed with, every open result and plaintext byte
once before the timing, and the host walk's entries against the device's.  One JSON line per workload.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hsig-picotls_amd"))
import ptls_hip  # noqa: E402

CIPHERS = {"aes128": (ptls_hip.ALGO_AESGCM, 16), "aes256": (ptls_hip.ALGO_AESGCM, 32),
           "chacha": (ptls_hip.ALGO_CHACHA20POLY1305, 32)}
NCONN = 1 << 16
HOST_DIR = os.path.join(ROOT, "tools", "quic_parse_host")
# (first byte, header bytes in front of the DCID, bytes behind it up to Length, payload, type, packet-number space)
SHORT = dict(first=0x43, long=False, payload=1350, type=ptls_hip.QUIC_TYPE_ONE_RTT, space=2)
WORKLOADS = {
    "short": dict(n=1 << 20, stride=1392, packets=[SHORT]),
    "coalesced": dict(n=1 << 18, stride=1360, packets=[
        dict(first=0xC3, long=True, token=True, payload=250, type=ptls_hip.QUIC_TYPE_INITIAL, space=0),
        dict(first=0xE3, long=True, token=False, payload=400, type=ptls_hip.QUIC_TYPE_HANDSHAKE, space=1),
        dict(SHORT, payload=600)]),
}


def host_lib():
    so = os.path.join(HOST_DIR, "libquic_parse_host.so")
    src = os.path.join(HOST_DIR, "quic_parse_host.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(ROOT, "hsig-picotls_amd", "csrc"), src, "-o", so])
    L = ctypes.CDLL(so)
    L.quic_parse_host.restype = ctypes.c_size_t
    L.quic_parse_host.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                  ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    L.quic_parse_host_map.restype = None
    L.quic_parse_host_map.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_size_t]
    return L


def headers(p, cid, pn):
    """(n, header bytes) of packet class p, unprotected, and pn_offset"""
    n = len(cid)
    pn4 = (pn & np.uint64(0xffffffff)).astype(">u4").view(np.uint8).reshape(n, 4)
    first = np.full((n, 1), p["first"], np.uint8)
    if not p["long"]:
        return np.concatenate([first, cid, pn4], axis=1), 9
    length = 4 + p["payload"] + 16
    fixed = bytes([0, 0, 0, 1, 8])
    tail = bytes([0]) + (bytes([0]) if p["token"] else b"") + bytes([0x40 | length >> 8, length & 0xff])
    parts = [first, np.tile(np.frombuffer(fixed, np.uint8), (n, 1)), cid, np.tile(np.frombuffer(tail, np.uint8), (n, 1)), pn4]
    h = np.concatenate(parts, axis=1)
    return h, h.shape[1] - 4


def median(v):
    return round(float(np.median(v)), 3)


def run(eng, name, args):
    w = WORKLOADS[name]
    n, stride = max(1, w["n"] // args.scale), w["stride"]
    nconn = min(NCONN, n)
    algo, ksz = CIPHERS[args.cipher]
    rng = np.random.default_rng(9000)
    idx = np.arange(n, dtype=np.uint64)
    conn = (idx % np.uint64(nconn)).astype(np.uint32)
    cids = ((np.arange(nconn, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)).astype(">u8").view(np.uint8).reshape(nconn, 8)
    ks, hp = ptls_hip.KeySet(eng, ksz, nconn, algo=algo), ptls_hip.KeySet(eng, ksz, nconn, algo=algo)
    ks.set(0, rng.integers(0, 256, nconn * ksz, dtype=np.uint8).tobytes(), rng.integers(0, 256, nconn * 12, dtype=np.uint8).tobytes())
    hp.set(0, rng.integers(0, 256, nconn * ksz, dtype=np.uint8).tobytes(), None)

    total = n * stride + 64
    d_pkt = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_pt = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")  # plaintext of a packet at its data_off
    seal, off = [], 0
    for p in w["packets"]:
        pn = idx + np.uint64(1 << 32) + np.uint64(p["space"] << 40)
        h, pn_offset = headers(p, cids[conn], pn)
        d_pkt[: n * stride].view(n, stride)[:, off: off + h.shape[1]].copy_(torch.from_numpy(h).cuda())
        pk = np.zeros(n, dtype=ptls_hip.QUIC_PACKET_DTYPE)
        pk["pkt_off"] = idx * np.uint64(stride) + np.uint64(off)
        pk["data_off"] = pk["pkt_off"] + np.uint64(pn_offset + 1)  # where the parse call will put the plaintext
        pk["pn"], pk["pkt_len"], pk["key"], pk["hp_key"] = pn, h.shape[1] + p["payload"] + 16, conn, conn
        pk["pn_offset"], pk["pn_len"] = pn_offset, 4
        seal.append(pk)
        off += int(pk["pkt_len"][0])
    dgram_len = off
    sealed = np.stack(seal, axis=1).reshape(-1)  # datagram order, wire order
    qs = ptls_hip.QuicBatch(eng, sealed, open=False)
    qs.seal(ks, hp, d_pt, d_pkt)
    torch.cuda.synchronize()
    qs.close()
    d_wire = d_pkt.clone()

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
    stream = torch.cuda.current_stream().cuda_stream

    def parse_into(pkts, info):
        got = ctypes.c_size_t(0)
        t0 = time.perf_counter()
        rc = L.ptls_hip_quic_parse_datagrams(eng.ptr, ctypes.addressof(params), cmap.ptr, dg.ctypes.data, n, d_pkt.data_ptr(),
                                             total, pkts.ctypes.data, info.ctypes.data, npk, ctypes.byref(got), stream)
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and got.value == npk, ptls_hip.last_error()
        k, d = ctypes.c_float(), ctypes.c_float()
        L.ptls_hip_quic_parse_timing(1, ctypes.byref(k), ctypes.byref(d))
        return ms, k.value, d.value

    def host_arrays(pinned):
        if not pinned:
            return np.zeros(npk, dtype=ptls_hip.QUIC_PACKET_DTYPE), np.zeros(npk, dtype=ptls_hip.QUIC_PKTINFO_DTYPE), None
        keep = (torch.zeros(npk * 40, dtype=torch.uint8).pin_memory(), torch.zeros(npk * 32, dtype=torch.uint8).pin_memory())
        return keep[0].numpy().view(ptls_hip.QUIC_PACKET_DTYPE), keep[1].numpy().view(ptls_hip.QUIC_PKTINFO_DTYPE), keep

    L.ptls_hip_quic_parse_timing(1, None, None)
    out = dict(workload=name, cipher=args.cipher, datagrams=n, packets=npk, datagram_bytes=dgram_len, cids=nconn,
               steps=args.steps, warmup=args.warmup)
    for pinned in (False, True):
        pkts, info, keep = host_arrays(pinned)
        t = [parse_into(pkts, info) for _ in range(args.warmup + args.steps)][args.warmup:]
        out["parse_pinned" if pinned else "parse_pageable"] = dict(call_ms=median([a for a, _, _ in t]),
                                                                   kernels_ms=median([b for _, b, _ in t]),
                                                                   d2h_ms=median([c for _, _, c in t]))
        pkts, info = pkts.copy(), info.copy()
        del keep
    L.ptls_hip_quic_parse_timing(0, None, None)
    # what was parsed is what was sealed
    for f in ("pkt_off", "data_off", "pkt_len", "key", "hp_key", "pn_offset"):
        assert np.array_equal(pkts[f], sealed[f]), f
    types = np.tile(np.array([p["type"] for p in w["packets"]], np.uint8), n)
    assert np.array_equal(info["type"], types) and (info["status"] == 0).all()
    assert np.array_equal(info["conn"], sealed["key"]) and np.array_equal(info["dgram"], np.repeat(idx.astype(np.uint32), len(w["packets"])))
    assert np.array_equal(pkts["pn"], expected[sealed["key"], np.tile(np.array([p["space"] for p in w["packets"]]), n)])

    # the same walk on one host core
    H = host_lib()
    h_buf = d_wire.cpu().numpy()
    size = 2
    while size < 2 * nconn:
        size <<= 1
    table = np.zeros(size * 32, dtype=np.uint8)
    packed = np.zeros((nconn, 20), np.uint8)
    packed[:, :8] = cids
    lens, conns = np.full(nconn, 8, np.uint8), np.arange(nconn, dtype=np.uint32)
    H.quic_parse_host_map(table.ctypes.data, size, packed.ctypes.data, lens.ctypes.data, conns.ctypes.data, nconn)
    hp_pkts, hp_info = np.zeros(npk, dtype=ptls_hip.QUIC_PACKET_DTYPE), np.zeros(npk, dtype=ptls_hip.QUIC_PKTINFO_DTYPE)
    host = []
    for _ in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        got = H.quic_parse_host(dg.ctypes.data, n, h_buf.ctypes.data, 8, 16, 1, table.ctypes.data, size, hp_pkts.ctypes.data,
                                hp_info.ctypes.data)
        host.append((time.perf_counter() - t0) * 1e3)
        assert got == npk
    assert np.array_equal(hp_info, info)
    hp_pkts["pn"] = pkts["pn"]
    assert np.array_equal(hp_pkts, pkts)
    out["host_walk_ms"] = median(host[args.warmup:])

    # plan and open what was parsed
    t0 = time.perf_counter()
    qo = ptls_hip.QuicBatch(eng, pkts, open=True)
    out["plan_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(npk, dtype=torch.int64, device="cuda")
    d_pn = torch.zeros(npk, dtype=torch.int64, device="cuda")
    recs = np.zeros(npk, dtype=ptls_hip.RECORD_DTYPE)
    hdr = sealed["pn_offset"].astype(np.uint64) + np.uint64(4)
    recs["aad_off"], recs["aad_len"], recs["in_off"], recs["out_off"] = sealed["pkt_off"], hdr, sealed["pkt_off"] + hdr, sealed["data_off"]
    recs["len"], recs["seq"], recs["key"] = sealed["pkt_len"] - hdr.astype(np.uint32) - 16, sealed["pn"], sealed["key"]
    bo = ptls_hip.Batch(eng, recs)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    st = torch.cuda.current_stream()
    opens, records = [], []
    for step in range(args.warmup + args.steps):
        d_pkt.copy_(d_wire)
        ev[0].record(st)
        qo.open(ks, hp, d_pkt, d_out, d_res, d_pn, st)
        ev[1].record(st)
        if step == 0:  # every result, packet number and plaintext byte, once
            torch.cuda.synchronize()
            assert np.array_equal(d_res.cpu().numpy().view(np.uint64), recs["len"].astype(np.uint64)), "an open failed"
            assert np.array_equal(d_pn.cpu().numpy().view(np.uint64), sealed["pn"])
            for pk, p in zip(seal, w["packets"]):
                o = int(pk["data_off"][0])
                a = d_out[: n * stride].view(n, stride)[:, o: o + p["payload"]]
                assert torch.equal(a, d_pt[: n * stride].view(n, stride)[:, o: o + p["payload"]]), "plaintext differs"
        ev[2].record(st)  # the headers in d_pkt are unprotected now: the record kernel alone, descriptors known
        if args.cipher == "chacha":
            bo.chacha_open(ks, d_pkt, d_pkt, d_out, d_res, st)
        else:
            bo.open(ks, d_pkt, d_pkt, d_out, d_res, st)
        ev[3].record(st)
        torch.cuda.synchronize()
        opens.append(ev[0].elapsed_time(ev[1]))
        records.append(ev[2].elapsed_time(ev[3]))
    out["open_ms"], out["record_ms"] = median(opens[args.warmup:]), median(records[args.warmup:])
    out["unprotect_ms"] = round(out["open_ms"] - out["record_ms"], 3)
    out["lanes"] = qo.records().chacha_lanes if args.cipher == "chacha" else qo.records().lanes
    qo.close()
    bo.close()
    cmap.close()
    ks.close()
    hp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1, help="divide the datagram counts (a quick run)")
    ap.add_argument("--cipher", default="aes128", choices=list(CIPHERS))
    ap.add_argument("--workload", default="all", choices=["all"] + list(WORKLOADS))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a gfx950 device"
    eng = ptls_hip.Engine(0)
    for name in (list(WORKLOADS) if args.workload == "all" else [args.workload]):
        print(json.dumps(run(eng, name, args)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
