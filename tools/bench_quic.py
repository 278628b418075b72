#!/usr/bin/env python3
"""QUIC packet protection with on-device header protection (ptls_hip_quic_seal_batch / _open_batch) next to the same packets
through the calls that existed before it, in one process on one clock (device-resident batches).

  python tools/bench_quic.py [--steps K] [--warmup W] [--packets N] [--cipher aes128|aes256|chacha|all]

Shape: N (default 1 048 576) short-header packets of 1 350 payload bytes, 13 header bytes (pn_offset 9, 4 packet-number
bytes) and the tag, 1 379 bytes each at a 1 392-byte stride; over 65 536 keys (packet i uses AEAD and header-protection key
i % 65 536) and over one key; AES-128-GCM, AES-256-GCM and ChaCha20-Poly1305.

  quic      seal = QuicBatch.seal (record + mask launch, then the header kernel); open = QuicBatch.open (the header kernel
            rewrites the descriptors, then the record launch).  Headers are protected on the wire image and come back
            unprotected, so every step starts from the same bytes.
  baseline  seal = seal_batch_supp (the masks stay in a side buffer: nobody applies them); open = aesecb_batch /
            chacha20_mask_batch over the same samples + open_batch with descriptors the host already knows (the packet-number
            length is given, the headers were never protected).  What could be done before, with the host round trip that
            unmasks and decodes the packet numbers left out.

Timing discipline of bench.py: W untimed warm-up steps (seal + open), a synchronize, then K steps; each step's seal and open
are bracketed by HIP events on the launch stream and the medians are reported (baseline.mask_ms: its stand-alone mask kernel
alone, the launch the open side's header kernel replaces).  GiB/s = payload bytes per second.  Every open
result, packet number and recovered byte is checked once before the timing.  One JSON line per cipher and key count.
"""
import argparse
import json
import os
import sys

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
DSTRIDE = (L + 15) & ~15
CIPHERS = {"aes128": (ptls_hip.ALGO_AESGCM, 16), "aes256": (ptls_hip.ALGO_AESGCM, 32),
           "chacha": (ptls_hip.ALGO_CHACHA20POLY1305, 32)}


def measure(step, steps, warmup, payload, with_mask=False):
    """with_mask: the step also records ev[3] after its stand-alone mask kernel (the first launch of its open side)"""
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for _ in range(warmup):
        step(stream, None)
    torch.cuda.synchronize()
    times, mask = [], []
    for _ in range(steps):
        step(stream, ev)
        torch.cuda.synchronize()
        times.append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
        if with_mask:
            mask.append(ev[1].elapsed_time(ev[3]))
    seal_ms = float(np.median([a for a, _ in times]))
    open_ms = float(np.median([b for _, b in times]))
    extra = dict(mask_ms=round(float(np.median(mask)), 3)) if with_mask else {}
    return dict(seal_gibps=round(payload / (seal_ms * 1e-3) / GIB, 1), open_gibps=round(payload / (open_ms * 1e-3) / GIB, 1),
                seal_open_gibps=round(2 * payload / ((seal_ms + open_ms) * 1e-3) / GIB, 1),
                seal_ms=round(seal_ms, 3), open_ms=round(open_ms, 3), **extra)


def run(eng, cipher, nkeys, args, bufs):
    algo, ksz = CIPHERS[cipher]
    n = args.packets
    d_pt, d_pkt, d_out, d_res, d_pn, d_mask, h_hdr = bufs
    idx = np.arange(n, dtype=np.uint64)
    pn = idx + np.uint64(1 << 32)  # unique per key, the nonce's upper half in use
    key = (idx % np.uint64(nkeys)).astype(np.uint32)
    rng = np.random.default_rng(9001)
    ks, hp = ptls_hip.KeySet(eng, ksz, nkeys, algo=algo), ptls_hip.KeySet(eng, ksz, nkeys, algo=algo)
    ks.set(0, rng.integers(0, 256, nkeys * ksz, dtype=np.uint8).tobytes(), rng.integers(0, 256, nkeys * 12, dtype=np.uint8).tobytes())
    hp.set(0, rng.integers(0, 256, nkeys * ksz, dtype=np.uint8).tobytes(), None)
    # the unprotected headers: short header, 4 packet-number bytes, an 8-byte connection ID
    h_hdr[:, 0] = 0x40 | (PN_LEN - 1)
    h_hdr[:, PN_OFFSET:] = (pn & np.uint64(0xffffffff)).astype(">u4").view(np.uint8).reshape(n, 4)
    v_hdr = d_pkt[: n * STRIDE].view(n, STRIDE)[:, :HDR]
    d_hdr = torch.from_numpy(h_hdr).cuda()
    d_pkt.zero_()
    v_hdr.copy_(d_hdr)
    v_pt, v_out = d_pt[: n * DSTRIDE].view(n, DSTRIDE)[:, :L], d_out[: n * DSTRIDE].view(n, DSTRIDE)[:, :L]
    d_pnv = torch.from_numpy(pn.astype(np.int64)).cuda()
    payload = float(n) * L

    def check(tag, with_pn):
        torch.cuda.synchronize()
        assert bool((d_res == L).all()), tag + ": an open failed"
        assert torch.equal(v_pt, v_out), tag + ": round trip differs"
        assert torch.equal(v_hdr, d_hdr), tag + ": the headers did not come back unprotected"
        if with_pn:
            assert torch.equal(d_pn, d_pnv), tag + ": packet numbers differ"
        d_out.zero_()
        d_res.zero_()
        d_pn.zero_()

    # the new calls
    pk = np.zeros(n, dtype=ptls_hip.QUIC_PACKET_DTYPE)
    pk["pkt_off"], pk["data_off"], pk["pn"] = idx * np.uint64(STRIDE), idx * np.uint64(DSTRIDE), pn
    pk["pkt_len"], pk["key"], pk["hp_key"], pk["pn_offset"], pk["pn_len"] = PKT, key, key, PN_OFFSET, PN_LEN
    qs = ptls_hip.QuicBatch(eng, pk, open=False)
    pk["pn"] = pn - np.uint64(1)  # the receiver has seen the packet before
    qo = ptls_hip.QuicBatch(eng, pk, open=True)

    def quic_step(stream, ev):
        if ev:
            ev[0].record(stream)
        qs.seal(ks, hp, d_pt, d_pkt, stream)
        if ev:
            ev[1].record(stream)
        qo.open(ks, hp, d_pkt, d_out, d_res, d_pn, stream)
        if ev:
            ev[2].record(stream)

    quic_step(torch.cuda.current_stream(), None)
    check(cipher + " quic", True)
    r_quic = measure(quic_step, args.steps, args.warmup, payload)
    r_quic["lanes"] = qo.records().chacha_lanes if cipher == "chacha" else qo.records().lanes
    qs.close()
    qo.close()

    # the calls that were there before, descriptors known to the host
    recs = np.zeros(n, dtype=ptls_hip.RECORD_DTYPE)
    recs["in_off"], recs["out_off"], recs["aad_off"] = pk["data_off"], pk["pkt_off"] + np.uint64(HDR), pk["pkt_off"]
    recs["seq"], recs["len"], recs["aad_len"], recs["key"] = pn, L, HDR, key
    orecs = recs.copy()
    orecs["in_off"], orecs["out_off"] = recs["out_off"], recs["in_off"]
    sp = np.zeros(n, dtype=ptls_hip.SUPP_DTYPE)
    sp["sample_off"], sp["mask_off"] = pk["pkt_off"] + np.uint64(PN_OFFSET + 4), idx * np.uint64(16)
    sp["hp_key"], sp["flags"] = key, ptls_hip.SUPP_ENABLE
    d_sp = torch.from_numpy(np.frombuffer(sp.tobytes(), np.uint8).copy()).cuda()
    bs, bo = ptls_hip.Batch(eng, recs), ptls_hip.Batch(eng, orecs)

    def base_step(stream, ev):
        if ev:
            ev[0].record(stream)
        if cipher == "chacha":
            bs.chacha_seal_supp(ks, hp, d_sp, d_pt, d_pkt, d_pkt, d_mask, stream)
        else:
            bs.seal_supp(ks, hp, d_sp, d_pt, d_pkt, d_pkt, d_mask, stream)
        if ev:
            ev[1].record(stream)
        if cipher == "chacha":
            eng.chacha20_mask(hp, d_sp, d_pkt, d_mask, stream)
            if ev:
                ev[3].record(stream)
            bo.chacha_open(ks, d_pkt, d_pkt, d_out, d_res, stream)
        else:
            eng.aesecb(hp, d_sp, d_pkt, d_mask, stream)
            if ev:
                ev[3].record(stream)
            bo.open(ks, d_pkt, d_pkt, d_out, d_res, stream)
        if ev:
            ev[2].record(stream)

    base_step(torch.cuda.current_stream(), None)
    check(cipher + " baseline", False)
    r_base = measure(base_step, args.steps, args.warmup, payload, with_mask=True)
    r_base["lanes"] = bo.chacha_lanes if cipher == "chacha" else bo.lanes
    bs.close()
    bo.close()
    ks.close()
    hp.close()
    return dict(cipher=cipher, packets=n, payload_bytes=L, packet_bytes=PKT, keys=nkeys, steps=args.steps, warmup=args.warmup,
                quic=r_quic, baseline=r_base,
                seal_ratio=round(r_quic["seal_gibps"] / r_base["seal_gibps"], 3),
                open_ratio=round(r_quic["open_gibps"] / r_base["open_gibps"], 3),
                seal_open_ratio=round(r_quic["seal_open_gibps"] / r_base["seal_open_gibps"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--cipher", default="all", choices=["all"] + list(CIPHERS))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a gfx950 device"
    eng = ptls_hip.Engine(0)
    n = args.packets
    rng = np.random.default_rng(1350)
    bufs = (torch.randint(0, 256, (n * DSTRIDE + 16,), dtype=torch.uint8, device="cuda"),
            torch.zeros(n * STRIDE + 16, dtype=torch.uint8, device="cuda"),
            torch.zeros(n * DSTRIDE + 16, dtype=torch.uint8, device="cuda"),
            torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda"),
            torch.zeros(n * 16, dtype=torch.uint8, device="cuda"),
            rng.integers(0, 256, (n, HDR), dtype=np.uint8))
    for cipher in (list(CIPHERS) if args.cipher == "all" else [args.cipher]):
        for nkeys in (1 << 16, 1):
            print(json.dumps(run(eng, cipher, min(nkeys, n), args, bufs)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
