"""The COPY host transport writes exactly the records' bytes into the caller's buffers.

fusion writes a record's output and nothing else (storen128 for the partial block, lib/fusion.c:388-397; the tag store,
:632).  The copy transport stages a slice's records through device buffers; it used to copy the slice's whole output span
back, so every byte lying between two records in the caller's buffer received whatever the staging held, e.g. the
plaintext of an earlier open on the same pipeline.  Here ONE copy-transport pipeline (pageable numpy buffers, as a socket
buffer would be) first opens records so that its staging holds plaintext, then seals, seals with QUIC header protection,
seals TLS 1.3 messages and opens again, every time into output buffers pre-filled with 0xA5 with 1-64-byte gaps between
the records: every record equals the oracle's (lib/fusion.c restated, pinned by tests/golden) and every other byte is
still 0xA5.  Cases: both key sizes; 64 KiB and 1 MiB slices; many records per slice (the gap-filled copies) and five
(one copy per record run); descriptors in output order and shuffled (a slice's gaps then hold other slices' records,
which must not be overwritten).

Every helper takes the kind of the caller's buffers ("pageable": numpy, as here; "pinned": page-locked memory, with which
the slices' copies really overlap, tests/test_gpu_copy_pinned.py) and the transport the call must have used, and compares
each WHOLE output and mask buffer with its expected image: the prefill with the oracle's bytes laid in.
"""
import numpy as np
import pytest
import torch

import ptls_hip

pytestmark = pytest.mark.gpu
FILL = 0xA5
COPY = ptls_hip.TRANSPORT_COPY
MASK_LAYOUTS = ("stride32", "perm32", "perm16")


class Bufs:
    """the caller's buffers of one call, pageable (numpy) or pinned (a page-locked torch tensor, kept alive here, used
    through its numpy view exactly as the numpy buffers are)"""

    def __init__(self, kind):
        assert kind in ("pageable", "pinned")
        self.kind, self.keep = kind, []

    def __call__(self, arr):
        """a NEW buffer of this kind with the contents (and dtype) of `arr`: what the pipeline writes never reaches `arr`,
        from which the expected image is built after the call"""
        if self.kind == "pageable":
            return arr.copy()
        t = torch.empty(arr.nbytes, dtype=torch.uint8).pin_memory()
        assert t.is_pinned()
        self.keep.append(t)
        view = t.numpy().view(arr.dtype)
        view[:] = arr
        return view


def _place(rng, sizes, gap_max):
    """offsets of back-to-back ranges of `sizes` with a 1..gap_max-byte gap before each one, and the buffer size"""
    off, pos = [], 0
    for s in sizes:
        pos += int(rng.integers(1, gap_max + 1))
        off.append(pos)
        pos += int(s)
    return off, pos + int(rng.integers(1, gap_max + 1))


def image(base, offs, pieces):
    """`base` with pieces[i] (bytes) laid in at offs[i]"""
    img = base.copy()
    for o, p in zip(offs, pieces):
        img[o: o + len(p)] = np.frombuffer(p, np.uint8)
    return img


def _same(got, want, what):
    """the WHOLE buffer equals its expected image"""
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (what, "%d bytes differ, first at" % diff.size, diff[:8].tolist())


def mask_prefill(size):
    """position-dependent, so mask bytes that come back at a wrong offset differ as well"""
    return ((7 + 131 * np.arange(size)) & 0xFF).astype(np.uint8)


class Case:
    def __init__(self, engine, oracle, bits, n, seed, lens=None, aad_len=13):
        """n records of the length mix below, or of the given `lens`"""
        self.aad_len = aad_len
        rng = np.random.default_rng(seed)
        self.rng = rng
        kb = bits // 8
        self.keys = [oracle.gen_key(70 + k, kb) for k in range(2)]
        self.ks = ptls_hip.KeySet(engine, kb, 2)
        self.ks.set(0, self.keys[0][0] + self.keys[1][0], self.keys[0][1] + self.keys[1][1])
        choices = [0, 1, 15, 16, 17, 100, 1350, 4095, 16384]
        self.lens = [int(rng.choice(choices)) if i % 3 else int(rng.integers(0, 3000)) for i in range(n)]
        if lens is not None:
            assert len(lens) == n
            self.lens = list(lens)
        self.key = [i * 2 // n for i in range(n)]  # two key runs
        self.seq = [1000 + i for i in range(n)]
        self.aad = [oracle.stream(500 + i, aad_len) for i in range(n)]
        self.pt = [oracle.stream(900 + i, L) for i, L in enumerate(self.lens)]
        self.sealed = [oracle.seal(*self.keys[self.key[i]], self.seq[i], self.aad[i], self.pt[i]) for i in range(n)]

    def recs(self, in_off, out_off, aad_off):
        n = len(self.lens)
        r = np.zeros(n, dtype=ptls_hip.RECORD_DTYPE)
        r["in_off"], r["out_off"], r["aad_off"] = in_off, out_off, aad_off
        r["seq"], r["len"], r["aad_len"], r["key"] = self.seq, self.lens, self.aad_len, self.key
        return r

    def aad_buffer(self):
        aad_off, size = _place(self.rng, [self.aad_len] * len(self.lens), 8)
        buf = self.rng.integers(0, 256, size, dtype=np.uint8)
        for o, a in zip(aad_off, self.aad):
            buf[o: o + self.aad_len] = np.frombuffer(a, np.uint8)
        return aad_off, buf

    def input_buffer(self, pieces):
        in_off, in_size = _place(self.rng, [len(p) for p in pieces], 4)
        return in_off, image(self.rng.integers(0, 256, in_size, dtype=np.uint8), in_off, pieces)


def _order(n, shuffled, rng):
    return rng.permutation(n) if shuffled else np.arange(n)


def _seal(case, pipe, gap_max, perm, kind="pageable", transport=COPY):
    bufs = Bufs(kind)
    in_off, h_in = case.input_buffer(case.pt)
    aad_off, h_aad = case.aad_buffer()
    out_off, out_size = _place(case.rng, [L + 16 for L in case.lens], gap_max)
    base = np.full(out_size, FILL, np.uint8)
    h_out = bufs(base)
    recs = case.recs(in_off, out_off, aad_off)
    pipe.seal(case.ks, recs[perm], bufs(h_in), bufs(h_aad), h_out)
    assert pipe.last_transport == transport
    for i, o in enumerate(out_off):
        assert h_out[o: o + case.lens[i] + 16].tobytes() == case.sealed[i], ("seal", i)
    _same(h_out, image(base, out_off, case.sealed), "seal wrote between records")
    return out_off, h_out


def _open(case, pipe, gap_max, perm, kind="pageable", transport=COPY):
    bufs = Bufs(kind)
    in_off, h_in = case.input_buffer(case.sealed)
    aad_off, h_aad = case.aad_buffer()
    out_off, out_size = _place(case.rng, case.lens, gap_max)
    base = np.full(out_size, FILL, np.uint8)
    h_out = bufs(base)
    h_res = bufs(np.zeros(len(case.lens), np.uint64))
    recs = case.recs(in_off, out_off, aad_off)
    pipe.open(case.ks, recs[perm], bufs(h_in), bufs(h_aad), h_out, h_res)
    assert pipe.last_transport == transport
    assert [int(x) for x in h_res] == [case.lens[i] for i in perm]
    for i, o in enumerate(out_off):
        assert h_out[o: o + case.lens[i]].tobytes() == case.pt[i], ("open", i)
    _same(h_out, image(base, out_off, case.pt), "open wrote between records")


def mask_offsets(n, layout):
    """(mask offset of every record, size of the mask buffer).  stride32: 32 i + 8 in record order, 16 untouched bytes
    between any two masks.  perm32: 32 q[i] + 8 for a fixed permutation q that does not depend on the descriptor order, so
    every slice's masks lie all over the buffer, between other slices' masks.  perm16: 16 q[i], packed: every byte of the
    buffer is some record's mask"""
    q = np.random.default_rng(4242).permutation(n)
    if layout == "far":  # 20 000 bytes from one mask to the next: a few masks span more than a 64 KiB slice
        return [20000 * i + 3 for i in range(n)], 20000 * n
    assert layout in MASK_LAYOUTS
    if layout == "stride32":
        return [32 * i + 8 for i in range(n)], 32 * n + 16
    if layout == "perm32":
        return [32 * int(q[i]) + 8 for i in range(n)], 32 * n + 16
    return [16 * int(q[i]) for i in range(n)], 16 * n


def _seal_supp(case, pipe, oracle, gap_max, perm, kind="pageable", transport=COPY, layout="stride32", edit=None):
    """seal + header-protection masks: every fifth entry disabled, a few naming an hp_key outside the one-slot keyset
    (skipped on the device): their mask bytes, like every byte between masks, keep the caller's contents.
    edit(supp, out_off) may spoil the descriptors of a call that is expected to be refused"""
    bufs = Bufs(kind)
    kb = len(case.keys[0][0])
    hp_key = oracle.stream(77, kb)
    hp = ptls_hip.KeySet(pipe.engine, kb, 1)
    hp.set(0, hp_key, None)
    n = len(case.lens)
    in_off, h_in = case.input_buffer(case.pt)
    aad_off, h_aad = case.aad_buffer()
    out_off, out_size = _place(case.rng, [L + 16 for L in case.lens], gap_max)
    base = np.full(out_size, FILL, np.uint8)
    h_out = bufs(base)
    mask_off, mask_size = mask_offsets(n, layout)
    mbase = mask_prefill(mask_size)
    h_mask = bufs(mbase)
    supp = np.zeros(n, dtype=ptls_hip.SUPP_DTYPE)
    moffs, masks = [], []
    for i in range(n):
        off = int(case.rng.integers(0, case.lens[i] + 1))  # the sample may cover the tag
        enabled = i % 5 != 2
        slot = 3 if i % 11 == 7 else 0  # 3: outside the keyset
        supp[i] = (out_off[i] + off, mask_off[i], slot, ptls_hip.SUPP_ENABLE if enabled else 0)
        if enabled and slot == 0:
            moffs.append(mask_off[i])
            masks.append(oracle.aes_ecb(hp_key, case.sealed[i][off: off + 16]))
    if edit is not None:
        edit(supp, out_off)
    recs = case.recs(in_off, out_off, aad_off)
    try:
        pipe.seal_supp(case.ks, hp, recs[perm], supp[perm], bufs(h_in), bufs(h_aad), h_out, h_mask)
    finally:
        hp.close()
    assert pipe.last_transport == transport
    _same(h_out, image(base, out_off, case.sealed), "seal_supp output")
    _same(h_mask, image(mbase, moffs, masks), "seal_supp masks (%s)" % layout)


@pytest.mark.parametrize("order", ["in_order", "shuffled"])
@pytest.mark.parametrize("n", [300, 5])
@pytest.mark.parametrize("slice_kib", [64, 1024])
@pytest.mark.parametrize("bits", [128, 256])
def test_copy_transport_writes_only_record_bytes(engine, oracle, bits, slice_kib, n, order):
    case = Case(engine, oracle, bits, n, seed=bits + slice_kib + n)
    perm = _order(n, order == "shuffled", case.rng)
    pipe = ptls_hip.Pipeline(engine, slice_kib << 10, transport=ptls_hip.TRANSPORT_COPY)
    _open(case, pipe, 64, perm)  # first: the staging now holds plaintext
    _seal(case, pipe, 64, perm)
    _seal_supp(case, pipe, oracle, 64, perm)
    _open(case, pipe, 64, perm)
    _seal(case, pipe, 1, perm)  # 1-byte gaps
    pipe.close()
    case.ks.close()


def test_copy_transport_auto_for_pageable_buffers(engine, oracle):
    """AUTO picks the copy transport for pageable buffers, with the same exact-bytes output"""
    case = Case(engine, oracle, 128, 120, seed=11)
    pipe = ptls_hip.Pipeline(engine, 64 << 10)
    _open(case, pipe, 32, np.arange(120))
    _seal(case, pipe, 32, np.arange(120))
    pipe.close()
    case.ks.close()


def _tls13(engine, oracle, slice_kib, kind="pageable", transport=COPY):
    """TLS 1.3 seal on one pipeline, then the open of those wire bytes: each message's records back to back (header,
    ciphertext, tag), messages 1-64 bytes apart in a 0xA5-filled wire buffer; the records equal ptls_send's framing
    restated (5-byte header as AAD, the content type appended, lib/picotls.c:696-715) and the bytes between messages stay
    0xA5.  The open parses every message's records out of the wire and writes their inner plaintexts (content + type
    byte), messages 1-64 bytes apart again, into a 0xA5-filled buffer"""
    bufs = Bufs(kind)
    rng = np.random.default_rng(slice_kib)
    key, iv = oracle.gen_key(5, 16)
    ks = ptls_hip.KeySet(engine, 16, 1)
    ks.set(0, key, iv)
    lens = [int(rng.integers(1, 40000)) for _ in range(40)]
    pts = [oracle.stream(40 + m, L) for m, L in enumerate(lens)]
    wire_sizes = [ptls_hip.lib().ptls_hip_tls13_wire_size(L) for L in lens]
    wire_off, wire_size = _place(rng, wire_sizes, 64)
    in_off, in_size = _place(rng, lens, 4)
    h_in = image(np.zeros(in_size, np.uint8), in_off, pts)
    msgs = np.zeros(len(lens), dtype=ptls_hip.TLS13_MESSAGE_DTYPE)
    seq, seqs = 0, []
    for m, L in enumerate(lens):
        msgs[m] = (in_off[m], wire_off[m], seq, L, 0, 23, 0)
        seqs.append(seq)
        seq += (L + 16383) // 16384
    recs = ptls_hip.tls13_frame(msgs)
    wbase = np.full(wire_size, FILL, np.uint8)
    h_wire = bufs(wbase)
    pipe = ptls_hip.Pipeline(engine, slice_kib << 10, transport=transport)
    pipe.tls13_seal(ks, recs, bufs(h_in), h_wire)
    assert pipe.last_transport == transport
    wires, inners = [], []
    for m, (L, p) in enumerate(zip(lens, pts)):
        w, s = b"", seqs[m]
        for c in range(0, L, 16384):
            chunk = p[c: c + 16384]
            hdr = bytes([0x17, 3, 3]) + (len(chunk) + 17).to_bytes(2, "big")
            w += hdr + oracle.seal(key, iv, s, hdr, chunk + b"\x17")
            s += 1
        assert len(w) == wire_sizes[m]
        assert h_wire[wire_off[m]: wire_off[m] + len(w)].tobytes() == w, m
        wires.append(w)
        inners.append(b"".join(p[c: c + 16384] + b"\x17" for c in range(0, L, 16384)))
    _same(h_wire, image(wbase, wire_off, wires), "tls13 seal wrote between messages")
    # open what was sealed: the records of every message parsed from the wire, their plaintexts 1-64 bytes apart
    pt_off, pt_size = _place(rng, [len(x) for x in inners], 64)
    orecs = np.concatenate([ptls_hip.tls13_parse(wires[m], wire_off=wire_off[m], key=0, seq=seqs[m], out_base=pt_off[m])[0]
                            for m in range(len(lens))])
    assert len(orecs) == len(recs)
    pbase = np.full(pt_size, FILL, np.uint8)
    h_pt = bufs(pbase)
    h_res = bufs(np.zeros(len(orecs), np.uint64))
    pipe.tls13_open(ks, orecs, h_wire, h_pt, h_res)
    assert pipe.last_transport == transport
    assert [int(x) for x in h_res] == [(int(r["len"]) - 1) | 23 << 56 for r in orecs]
    _same(h_pt, image(pbase, pt_off, inners), "tls13 open wrote between messages")
    pipe.close()
    ks.close()


@pytest.mark.parametrize("slice_kib", [64, 1024])
def test_copy_transport_tls13_seal_gaps_between_messages(engine, oracle, slice_kib):
    _tls13(engine, oracle, slice_kib)
