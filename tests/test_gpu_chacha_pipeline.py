"""ChaCha20-Poly1305 through the host pipelines (ptls_hip_pipeline_new_algo; hsig-picotls_amd/csrc/pipeline.cpp,
chacha_kernel.hip on the copy transport's staging, chacha_runs_kernel.hip on the mapped transport), bit-exact against the
plain-Python RFC 8439 reference (tests/chacha_ref.py).  No tolerance anywhere.

Outputs go into 0xA5-filled and masks into 0x5A-filled buffers with 1- to 64-byte gaps between the records, and the WHOLE
output, mask and result buffers are compared with their expected images, so a byte written outside a record fails the test
that wrote it.  The reference images are computed once per module (about 330 KB of records for the plain calls, as much for
the TLS 1.3 ones, 200 KB for the width cases) and shared by every transport, order and kernel."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import chacha_ref
import ptls_hip

pytestmark = pytest.mark.gpu
U64 = (1 << 64) - 1
FILL, MASK_FILL = 0xA5, 0x5A
SLICE = 64 << 10
NK = 3
COPY, MAPPED = ptls_hip.TRANSPORT_COPY, ptls_hip.TRANSPORT_MAPPED
CHACHA = ptls_hip.ALGO_CHACHA20POLY1305
BLOCKS, RUNS = ptls_hip.CHACHA_LAYOUT_BLOCKS, ptls_hip.CHACHA_LAYOUT_RUNS
# buffers x transport asked for -> transport used
TRANSPORTS = {"pageable": (False, None, COPY), "copy_pinned": (True, COPY, COPY), "mapped": (True, MAPPED, MAPPED)}

LENS = ([0, 1, 15, 16, 63, 64, 65, 255, 256, 257, 1350, 4096, 16384] + [16384] * 15 + [1350] * 8 + [4096] * 4 +
        [700, 100, 1351, 8191, 1024, 1025, 4113, 2048, 33, 5, 640, 1279] + [1350] * 8)
N = len(LENS)
AADS = [0, 5, 13, 40]
SEQS = [0, 1, (1 << 32) - 1, 1 << 32, U64]
BAD = 17  # the record whose tag the open cases damage
# TLS 1.3: content lengths; with the content type the inner plaintexts of 63, 255, 4095, 16383, ... are multiples of 64
TLS_LENS = [max(1, L - 1) for L in LENS[:-3]] + [16384, 16384, 62]
TYPES = [23, 22, 21]


def stream(tag, n):
    out, i = bytearray(), 0
    while len(out) < n:
        out += hashlib.sha256(b"%s/%d" % (tag.encode(), i)).digest()
        i += 1
    return bytes(out[:n])


KEYS = [stream("pipe-chacha-key-%d" % i, 32) for i in range(NK)]
IVS = [bytes(b | 1 for b in stream("pipe-chacha-iv-%d" % i, 12)) for i in range(NK)]
HP_KEYS = [stream("pipe-chacha-hp-%d" % i, 32) for i in range(NK)]
PAYLOAD = stream("pipe-chacha-payload", 17000 + N)
AAD = stream("pipe-chacha-aad", 64)


@functools.lru_cache(maxsize=None)
def ref_seal(slot, seq, aad, pt):
    return chacha_ref.seal(KEYS[slot], IVS[slot], seq, aad, pt)


class Bufs:
    """host buffers of one case: pageable numpy copies, or views of pinned torch tensors (kept alive here)"""

    def __init__(self, pinned):
        self.pinned, self.keep = pinned, []

    def __call__(self, arr):
        if not self.pinned:
            return arr.copy()
        t = torch.empty(max(arr.nbytes, 1), dtype=torch.uint8).pin_memory()
        assert t.is_pinned()
        self.keep.append(t)
        view = t.numpy()[: arr.nbytes].view(arr.dtype)
        view[:] = arr
        return view


def place(sizes, step=None):
    """offsets of consecutive pieces: gaps of 1 .. 64 bytes; or packed with 1-byte gaps (step 1) / on multiples of 16 (16)"""
    offs, pos = [], 0
    for i, s in enumerate(sizes):
        if step is None:
            pos += 1 + (i * 7) % 64
        elif step == 1:
            pos += 1
        else:
            pos = (pos + 15) & ~15
        offs.append(pos)
        pos += s
    return offs, pos + 64


def image(base, offs, pieces):
    img = base.copy()
    for o, p in zip(offs, pieces):
        img[o: o + len(p)] = np.frombuffer(p, np.uint8)
    return img


def filled(size, value=FILL):
    return np.full(size, value, np.uint8)


def same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {int(bad[0])}")


def order_of(n, shuffled):
    return np.random.default_rng(n).permutation(n) if shuffled else np.arange(n)


@pytest.fixture(scope="module")
def keysets(engine):
    ks = ptls_hip.KeySet(engine, 32, NK, algo=CHACHA)
    ks.set(0, b"".join(KEYS), b"".join(IVS))
    hp = ptls_hip.KeySet(engine, 32, NK, algo=CHACHA)
    hp.set(0, b"".join(HP_KEYS), None)
    yield ks, hp
    ks.close()
    hp.close()


class Plain:
    """the records of the plain calls and their reference seals"""

    def __init__(self, lens, aad_of, step=None):
        self.n = len(lens)
        self.slot = [i % NK for i in range(self.n)]
        self.seq = [SEQS[i % 5] for i in range(self.n)]
        self.aad = [AAD[: aad_of(i)] for i in range(self.n)]
        self.pt = [PAYLOAD[i: i + L] for i, L in enumerate(lens)]
        self.sealed = [ref_seal(self.slot[i], self.seq[i], self.aad[i], self.pt[i]) for i in range(self.n)]
        self.pt_off, self.pt_size = place(lens, step)
        self.ct_off, self.ct_size = place([L + 16 for L in lens], step)
        self.aad_off, self.aad_size = place([len(a) for a in self.aad], step)
        self.h_aad = image(np.zeros(self.aad_size, np.uint8), self.aad_off, self.aad)

    def recs(self, in_off, out_off):
        d = np.zeros(self.n, dtype=ptls_hip.RECORD_DTYPE)
        d["in_off"], d["out_off"], d["aad_off"] = in_off, out_off, self.aad_off
        d["seq"] = np.array(self.seq, dtype=np.uint64)
        d["len"], d["aad_len"], d["key"] = [len(p) for p in self.pt], [len(a) for a in self.aad], self.slot
        return d


@pytest.fixture(scope="module")
def plain():
    assert 300_000 <= sum(LENS) <= 400_000 and N == 60  # the mapped transport cuts two slices of 4 x 64 KiB, the copy one six
    return Plain(LENS, lambda i: AADS[i % 4])


def run_seal(case, ks, pipe, bufs, perm, used, what="seal"):
    h_in = bufs(image(np.zeros(case.pt_size, np.uint8), case.pt_off, case.pt))
    h_out = bufs(filled(case.ct_size))
    pipe.seal(ks, case.recs(case.pt_off, case.ct_off)[perm], h_in, bufs(case.h_aad), h_out)
    assert pipe.last_transport == used
    same(h_out, image(filled(case.ct_size), case.ct_off, case.sealed), what)


def run_open(case, ks, pipe, bufs, perm, used, bad=None, what="open"):
    inputs = list(case.sealed)
    if bad is not None:
        x = bytearray(inputs[bad])
        x[len(case.pt[bad]) + bad % 16] ^= 0x40
        inputs[bad] = bytes(x)
    h_in = bufs(image(np.zeros(case.ct_size, np.uint8), case.ct_off, inputs))
    h_out = bufs(filled(case.pt_size))
    h_res = bufs(np.full(case.n, 7, np.uint64))
    pipe.open(ks, case.recs(case.ct_off, case.pt_off)[perm], h_in, bufs(case.h_aad), h_out, h_res)
    assert pipe.last_transport == used
    assert [int(x) for x in h_res] == [U64 if i == bad else len(case.pt[i]) for i in perm], what
    same(h_out, image(filled(case.pt_size), case.pt_off, case.pt), what)  # the damaged record's plaintext is written too


def run_seal_supp(case, ks, hp, pipe, bufs, perm, used):
    n = case.n
    rel = [len(case.pt[i]) if i % 4 == 0 else (i * 5) % (len(case.pt[i]) + 1) for i in range(n)]  # i % 4 == 0: the tag
    assert any(r == len(p) for r, p in zip(rel, case.pt)) and all(r <= len(p) for r, p in zip(rel, case.pt))
    # a slice's masks lie between other slices' masks: record i's is the (37 i mod n)-th, 20 bytes apart at odd offsets
    assert np.gcd(37, n) == 1
    mask_off = [3 + 20 * ((37 * i) % n) for i in range(n)]
    sp = np.zeros(n, dtype=ptls_hip.SUPP_DTYPE)
    sp["sample_off"] = [o + r for o, r in zip(case.ct_off, rel)]
    sp["mask_off"], sp["hp_key"], sp["flags"] = mask_off, [i % NK for i in range(n)], ptls_hip.SUPP_ENABLE
    skipped = set()
    for i in range(n):
        if i % 11 == 7:
            sp["flags"][i] = 0
            skipped.add(i)
        elif i % 13 == 5:
            sp["hp_key"][i] = NK + i
            skipped.add(i)
    want = [bytes([MASK_FILL]) * 16 if i in skipped else chacha_ref.hp_mask(HP_KEYS[i % NK], case.sealed[i][rel[i]: rel[i] + 16])
            for i in range(n)]
    mask_size = 20 * n + 64
    h_in = bufs(image(np.zeros(case.pt_size, np.uint8), case.pt_off, case.pt))
    h_out, h_mask = bufs(filled(case.ct_size)), bufs(filled(mask_size, MASK_FILL))
    pipe.seal_supp(ks, hp, case.recs(case.pt_off, case.ct_off)[perm], sp[perm], h_in, bufs(case.h_aad), h_out, h_mask)
    assert pipe.last_transport == used
    same(h_out, image(filled(case.ct_size), case.ct_off, case.sealed), "seal_supp records")
    same(h_mask, image(filled(mask_size, MASK_FILL), mask_off, want), "seal_supp masks")


class Tls:
    """one TLS 1.3 record per message (messages of at most 16384 bytes): the wire records and the inner plaintexts"""

    def __init__(self):
        self.n = len(TLS_LENS)
        self.slot = [i % NK for i in range(self.n)]
        self.seq = [SEQS[i % 5] for i in range(self.n)]
        self.type = [TYPES[i % 3] for i in range(self.n)]
        self.pt = [PAYLOAD[i: i + L] for i, L in enumerate(TLS_LENS)]
        self.inner = [p + bytes([t]) for p, t in zip(self.pt, self.type)]
        self.wire = []
        for i, inner in enumerate(self.inner):
            hdr = b"\x17\x03\x03" + (len(inner) + 16).to_bytes(2, "big")
            self.wire.append(hdr + ref_seal(self.slot[i], self.seq[i], hdr, inner))
        self.in_off, self.in_size = place(TLS_LENS)
        self.wire_off, self.wire_size = place([len(w) for w in self.wire])
        self.pt_off, self.pt_size = place([len(x) for x in self.inner])


@pytest.fixture(scope="module")
def tls():
    t = Tls()
    assert sum(1 for x in t.inner if len(x) % 64 == 0) >= 5 and sum(TLS_LENS) >= 300_000
    return t


def run_tls13_seal(t, ks, pipe, bufs, perm, used):
    msgs = np.zeros(t.n, dtype=ptls_hip.TLS13_MESSAGE_DTYPE)
    for i in range(t.n):
        msgs[i] = (t.in_off[i], t.wire_off[i], t.seq[i], TLS_LENS[i], t.slot[i], t.type[i], 0)
    recs = ptls_hip.tls13_frame(msgs)
    assert len(recs) == t.n
    h_wire = bufs(filled(t.wire_size))
    pipe.tls13_seal(ks, recs[perm], bufs(image(np.zeros(t.in_size, np.uint8), t.in_off, t.pt)), h_wire)
    assert pipe.last_transport == used
    same(h_wire, image(filled(t.wire_size), t.wire_off, t.wire), "tls13 seal")


def run_tls13_open(t, ks, pipe, bufs, perm, used):
    wires = list(t.wire)
    x = bytearray(wires[BAD])
    x[-1 - BAD % 16] ^= 0x01
    wires[BAD] = bytes(x)
    parsed = [ptls_hip.tls13_parse(t.wire[i], wire_off=t.wire_off[i], key=t.slot[i], seq=t.seq[i], out_base=t.pt_off[i])
              for i in range(t.n)]
    assert all(c == len(t.wire[i]) and len(r) == 1 for i, (r, c) in enumerate(parsed))
    recs = np.concatenate([r for r, _ in parsed])
    h_pt = bufs(filled(t.pt_size))
    h_res = bufs(np.full(t.n, 7, np.uint64))
    pipe.tls13_open(ks, recs[perm], bufs(image(np.zeros(t.wire_size, np.uint8), t.wire_off, wires)), h_pt, h_res)
    assert pipe.last_transport == used
    assert [int(v) for v in h_res] == [U64 if i == BAD else TLS_LENS[i] | t.type[i] << 56 for i in perm]
    same(h_pt, image(filled(t.pt_size), t.pt_off, t.inner), "tls13 open")


@pytest.mark.parametrize("shuffled", [False, True], ids=["in_order", "shuffled"])
@pytest.mark.parametrize("transport", list(TRANSPORTS))
@pytest.mark.parametrize("call", ["seal", "open", "seal_supp", "tls13_seal", "tls13_open"])
def test_every_call_on_every_transport(engine, keysets, plain, tls, call, transport, shuffled):
    """60 records over 3 key slots through a 64 KiB pipeline (the copy transport keeps three slices in flight and cuts six
    or more; the mapped one cuts two): whole buffers against the reference's images"""
    ks, hp = keysets
    pinned, asked, used = TRANSPORTS[transport]
    bufs = Bufs(pinned)
    perm = order_of(N, shuffled)
    pipe = ptls_hip.Pipeline(engine, SLICE, transport=asked, algo=CHACHA)
    assert pipe.algo == CHACHA
    if call == "seal":
        run_seal(plain, ks, pipe, bufs, perm, used)
    elif call == "open":
        run_open(plain, ks, pipe, bufs, perm, used, bad=BAD)
    elif call == "seal_supp":
        run_seal_supp(plain, ks, hp, pipe, bufs, perm, used)
    elif call == "tls13_seal":
        run_tls13_seal(tls, ks, pipe, bufs, perm, used)
    else:
        run_tls13_open(tls, ks, pipe, bufs, perm, used)
    pipe.close()


def width_lens(g):
    return [64 * nfull + tail for nfull in (0, 1, g - 1, g, g + 1, 2 * g - 1, 2 * g, 2 * g + 1) for tail in (0, 1, 17, 63)]


@pytest.mark.parametrize("step", [1, 16], ids=["packed1", "packed16"])
@pytest.mark.parametrize("g", [4, 16, 64])
def test_runs_kernel_at_each_width(engine, keysets, g, step):
    """the run-layout kernel forced at g lanes on the mapped transport: 32 records of 0 .. 2 g + 1 whole blocks with tails
    of 0, 1, 17 and 63 bytes, in this order (the groups of one wave then run different trip counts at g = 4 and 16), seal and
    open; the same records through the block kernel at 1 and g lanes"""
    ks, _ = keysets
    case = Plain(width_lens(g), lambda i: 13, step)
    assert case.n == 32
    bufs = Bufs(True)
    perm = np.arange(case.n)
    pipe = ptls_hip.Pipeline(engine, SLICE, transport=MAPPED, algo=CHACHA)
    for lanes, layout in ((g, RUNS), (1, BLOCKS), (g, BLOCKS)):
        pipe.set_chacha_lanes(lanes, layout)
        run_seal(case, ks, pipe, bufs, perm, MAPPED, f"seal lanes {lanes} layout {layout}")
        run_open(case, ks, pipe, bufs, perm, MAPPED, bad=9, what=f"open lanes {lanes} layout {layout}")
    pipe.close()


def test_refusals_and_the_unchanged_aes_path(engine, oracle, keysets, plain):
    """a ChaCha pipeline refuses AES keysets (and an AES header-protection keyset) with EINVAL and writes nothing, then serves
    a correct call; a pipeline from _new_algo(AESGCM) is the one ptls_hip_pipeline_new makes"""
    L = ptls_hip.lib()
    ks, hp = keysets
    aes = ptls_hip.KeySet(engine, 32, NK)
    aes.set(0, b"".join(KEYS), b"".join(IVS))
    small = Plain([100, 33, 1350, 0, 64], lambda i: 5)
    recs = small.recs(small.pt_off, small.ct_off)
    sp = np.zeros(small.n, dtype=ptls_hip.SUPP_DTYPE)
    sp["sample_off"], sp["mask_off"], sp["flags"] = small.ct_off, [16 * i for i in range(small.n)], ptls_hip.SUPP_ENABLE
    for pinned in (False, True):
        bufs = Bufs(pinned)
        pipe = ptls_hip.Pipeline(engine, SLICE, algo=CHACHA)
        h_in = bufs(image(np.zeros(small.ct_size, np.uint8), small.pt_off, small.pt))
        h_aad, h_out = bufs(small.h_aad), bufs(filled(small.ct_size))
        h_mask, h_res = bufs(filled(256, MASK_FILL)), bufs(np.full(small.n, 7, np.uint64))
        q = lambda a: a.ctypes.data  # noqa: E731
        n = small.n
        calls = [
            L.ptls_hip_pipeline_seal(pipe.ptr, aes.ptr, q(recs), n, q(h_in), q(h_aad), q(h_out)),
            L.ptls_hip_pipeline_open(pipe.ptr, aes.ptr, q(recs), n, q(h_in), q(h_aad), q(h_out), q(h_res)),
            L.ptls_hip_pipeline_seal_supp(pipe.ptr, aes.ptr, aes.ptr, q(recs), q(sp), n, q(h_in), q(h_aad), q(h_out), q(h_mask)),
            L.ptls_hip_pipeline_seal_supp(pipe.ptr, aes.ptr, hp.ptr, q(recs), q(sp), n, q(h_in), q(h_aad), q(h_out), q(h_mask)),
            L.ptls_hip_pipeline_seal_supp(pipe.ptr, ks.ptr, aes.ptr, q(recs), q(sp), n, q(h_in), q(h_aad), q(h_out), q(h_mask)),
            L.ptls_hip_pipeline_tls13_seal(pipe.ptr, aes.ptr, q(recs), n, q(h_in), q(h_out)),
            L.ptls_hip_pipeline_tls13_open(pipe.ptr, aes.ptr, q(recs), n, q(h_in), q(h_out), q(h_res)),
        ]
        assert calls == [ptls_hip.EINVAL] * len(calls)
        assert "ChaCha20-Poly1305 keysets" in ptls_hip.last_error()
        assert bool((h_out == FILL).all()) and bool((h_mask == MASK_FILL).all()) and bool((h_res == 7).all())
        # the setter's argument rules
        assert L.ptls_hip_pipeline_set_chacha_lanes(pipe.ptr, 3, 0) == ptls_hip.EINVAL
        assert L.ptls_hip_pipeline_set_chacha_lanes(pipe.ptr, 4, 3) == ptls_hip.EINVAL
        assert L.ptls_hip_pipeline_set_chacha_lanes(pipe.ptr, 1, RUNS) == ptls_hip.EINVAL
        assert L.ptls_hip_pipeline_set_chacha_lanes(pipe.ptr, 0, RUNS) == 0
        assert L.ptls_hip_pipeline_set_chacha_lanes(pipe.ptr, 0, 0) == 0
        used = MAPPED if pinned else COPY
        run_seal(small, ks, pipe, bufs, np.arange(n), used)
        run_open(small, ks, pipe, bufs, np.arange(n), used)
        pipe.close()
    # AES-GCM: both constructors, the same bytes (and the CPU oracle's)
    old, new = ptls_hip.Pipeline(engine, SLICE), ptls_hip.Pipeline(engine, SLICE, algo=ptls_hip.ALGO_AESGCM)
    assert old.algo == new.algo == ptls_hip.ALGO_AESGCM
    assert L.ptls_hip_pipeline_set_chacha_lanes(old.ptr, 4, 0) == ptls_hip.EINVAL
    assert L.ptls_hip_pipeline_set_chacha_lanes(new.ptr, 4, 0) == ptls_hip.EINVAL
    twenty = Plain(LENS[:13] + [1350] * 7, lambda i: AADS[i % 4])
    assert twenty.n == 20
    aes_sealed = [oracle.seal(KEYS[twenty.slot[i]], IVS[twenty.slot[i]], twenty.seq[i], twenty.aad[i], twenty.pt[i])
                  for i in range(twenty.n)]
    for pinned in (False, True):
        outs = []
        for pipe in (old, new):
            bufs = Bufs(pinned)
            h_out = bufs(filled(twenty.ct_size))
            pipe.seal(aes, twenty.recs(twenty.pt_off, twenty.ct_off), bufs(image(np.zeros(twenty.pt_size, np.uint8), twenty.pt_off,
                                                                                 twenty.pt)), bufs(twenty.h_aad), h_out)
            h_pt, h_res = bufs(filled(twenty.pt_size)), bufs(np.full(twenty.n, 7, np.uint64))
            pipe.open(aes, twenty.recs(twenty.ct_off, twenty.pt_off), h_out, bufs(twenty.h_aad), h_pt, h_res)
            assert [int(x) for x in h_res] == [len(p) for p in twenty.pt]
            outs.append((h_out.copy(), h_pt.copy(), pipe.last_transport))
        same(outs[0][0], outs[1][0], "AES seal through both constructors")
        same(outs[0][1], outs[1][1], "AES open through both constructors")
        assert outs[0][2] == outs[1][2] == (MAPPED if pinned else COPY)
        same(outs[0][0], image(filled(twenty.ct_size), twenty.ct_off, aes_sealed), "AES seal")
        same(outs[0][1], image(filled(twenty.pt_size), twenty.pt_off, twenty.pt), "AES open")
    # a ChaCha keyset on either AES pipeline: refused as before
    h = filled(twenty.ct_size)
    for pipe in (old, new):
        assert L.ptls_hip_pipeline_seal(pipe.ptr, ks.ptr, twenty.recs(twenty.pt_off, twenty.ct_off).ctypes.data, 20, h.ctypes.data,
                                        twenty.h_aad.ctypes.data, h.ctypes.data) == ptls_hip.EINVAL
        pipe.close()
    assert bool((h == FILL).all())
    aes.close()
