"""The seal-side exact-bytes matrix through the AES-GCM batch API on the device (used by tests/test_gpu_seal_exact.py;
the helpers are checked without a GPU by tests/test_seal_exact_helpers.py).

One `run` is one seal launch over explicit ptls_hip.RECORD_DTYPE descriptors into an output buffer pre-filled with 0xA5,
and compares WHOLE buffers with the CPU oracle's (oracle.seal, oracle.aes_ecb) images:

  * the output buffer equals the prefill with the oracle's ct || tag laid in at every out_off: a store that is misplaced,
    late into a neighbour's line, of zeros, or one byte too long shows as a byte "outside every record";
  * not in place, the input and the AAD buffer are unchanged; in place (out == in, one layout for both, random bytes in
    its gaps) the buffer equals its image before the launch with ct || tag laid over every record;
  * with header protection, the mask buffer equals its position-dependent prefill with AES-ECB(hp key, sample) laid in
    for the enabled entries that name a key of the keyset, and nothing else;
  * the sealed image is then opened into a fresh 0xA5 buffer with a sentinel-filled `result`: the whole plaintext image
    and every result.

Layouts (`layout`): "lines" (every offset a multiple of 16, so the ALIGNED instantiation runs; record i's output starts at
block lo = i mod 8 of a 128-byte line; 16..112 fill bytes between one record's tag and the next record's first byte in
address order, so a stray whole-block store lands in fill and not in a neighbour whose own store could race it away),
"packed16" (ptls_hip.layout_records, align 16), "bytes" (1..64 random bytes before each record: the unaligned
instantiation) and "packed1" (no gaps at all).

Shapes: `batch_shapes(G)` crosses L = 16 k + r, k around every multiple of the stretch iteration (2 G blocks:
PURE_BLOCKS = 2), with r and lo; `sparse_shapes()` walks the GHASH element counts of the lanes = 64 kernel.  Every
seventh record carries PTLS_HIP_RECORD_TLS13_TYPE (its last plaintext byte is the type, not input: the input holds a
poison byte there, which a kernel that read it would carry into ciphertext and tag).

Run as a script (`python seal_exact_case.py LANES KEY_LEN`) it prints, for whichever libptls_hip.so PTLS_HIP_LIB names,
one MISMATCHES line for the "lines" layout: the test runs it on the TEST-ONLY mutant build
(hsig-picotls_amd/mutants/libptls_hip_seal1.so, batch_kernel.h SEAL_MUTANT) and expects exactly one stray byte per record,
right behind its tag.
"""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "hsig-picotls_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ptls_hip  # noqa: E402

UINT64_MAX = (1 << 64) - 1
SENTINEL = 0x5A5A5A5A5A5A5A5A  # `result` before the open launch: neither a length nor UINT64_MAX
FILL = 0xA5
POISON = 0xEE  # the input byte at L - 1 of a record with a content type: never read
TAIL = 32      # fill bytes behind the last range of every buffer
BATCH_GS = (1, 2, 4, 8, 16, 32)
SPARSE_LANES = 64
PURE_BLOCKS = 2  # batch_kernel.h: one stretch iteration moves PURE_BLOCKS * G blocks of a record
RS = (0, 1, 5, 15)
LAYOUTS = ("lines", "packed16", "bytes", "packed1")
SPARSE_N = (1, 2, 41, 63, 64, 65, 66, 128, 129, 130, 154, 257)  # GHASH elements: no Horner step, the first, two, more
SPARSE_AADS = (0, 21)
TLS_TYPES = (21, 22, 23)

# L, A: payload and AAD bytes; key: key slot; ctype: TLS 1.3 content type or None
Shape = namedtuple("Shape", "L A key ctype")
# offsets per record and buffer sizes; in place, in_off is out_off and in_size is out_size
Layout = namedtuple("Layout", "in_off out_off aad_off in_size out_size aad_size")
# shapes; keys[slot] = (key, iv); seqs, aads, inputs (the input bytes, poison included), plains (what is sealed, what open
# returns) and sealed (the oracle's ct || tag) per record
Case = namedtuple("Case", "shapes keys seqs aads inputs plains sealed")


def batch_ks(G):
    """full blocks of the record lengths at G lanes per record: zero to three stretch iterations and both sides of each"""
    return sorted({0, 1, G - 1, G, G + 1, 2 * G, 2 * G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 5 * G + 1, 6 * G, 6 * G + 1})


def batch_aads(G):
    """the lanes' first data elements rotated by 0, 1, 1, 2 and G + 1 blocks"""
    return (0, 5, 16, 21, 16 * G + 3)


def _ctype(i, L):
    return TLS_TYPES[(i // 7) % 3] if i % 7 == 3 and L > 0 else None  # (a record of no bytes has no last byte)


def batch_shapes(G):
    """k x r x lo, lo innermost: record i of the list has i mod 8 == lo.  Two key runs; each holds every k and every lo"""
    aads = batch_aads(G)
    out = []
    for key in (0, 1):
        for k in batch_ks(G):
            for r in RS[2 * key: 2 * key + 2]:
                for _lo in range(8):
                    i = len(out)
                    out.append(Shape(16 * k + r, aads[i % len(aads)], key, _ctype(i, 16 * k + r)))
    return out


def ghash_elements(L, A):
    return (A + 15) // 16 + (L + 15) // 16 + 1


def sparse_shapes(reps=3):
    """the lanes = 64 kernel: every N of SPARSE_N with r in RS and AAD in SPARSE_AADS where such a length exists, a key per
    record; the list is repeated so that every shape meets several lo (its length is no multiple of 8)"""
    base = []
    for N in SPARSE_N:
        for A in SPARSE_AADS:
            nc = N - 1 - (A + 15) // 16
            if nc < 0:
                continue
            for r in RS if nc else RS[:1]:
                base.append((16 * nc if r == 0 else 16 * (nc - 1) + r, A))
    assert len(base) % 8 != 0
    out = []
    for _ in range(reps):
        for L, A in base:
            i = len(out)
            assert ghash_elements(L, A) in SPARSE_N
            out.append(Shape(L, A, i, _ctype(i, L)))
    return out


def shapes_for(lanes):
    return sparse_shapes() if lanes == SPARSE_LANES else batch_shapes(lanes)


@functools.lru_cache(maxsize=None)
def case(oracle, key_len, lanes):
    """the records of `lanes` and the oracle's seal of each, computed once per (key size, lanes)"""
    shapes = tuple(shapes_for(lanes))
    keys = tuple(oracle.gen_key(3100 + j, key_len) for j in range(max(s.key for s in shapes) + 1))
    seqs, aads, inputs, plains, sealed = [], [], [], [], []
    for i, s in enumerate(shapes):
        pt = oracle.stream(8200 + 1000 * lanes + i, s.L)
        seqs.append(0x0123456789AB0000 + i)
        aads.append(oracle.stream(9300 + 1000 * lanes + i, s.A))
        inputs.append(pt if s.ctype is None else pt[:-1] + bytes([POISON]))
        plains.append(pt if s.ctype is None else pt[:-1] + bytes([s.ctype]))
        sealed.append(oracle.seal(*keys[s.key], seqs[-1], aads[-1], plains[-1]))
    return Case(shapes, keys, tuple(seqs), tuple(aads), tuple(inputs), tuple(plains), tuple(sealed))


# ---------------------------------------------------------------------------------------------------------------------
# layouts


def _packed(sizes, align):
    off, pos = [], 0
    for s in sizes:
        pos = (pos + align - 1) // align * align
        off.append(pos)
        pos += s
    return off, (pos + align - 1) // align * align + TAIL


def _place(rng, sizes, gap_max):
    """back-to-back ranges with a 1..gap_max-byte gap before each one (as tests/test_gpu_copy_gaps.py)"""
    off, pos = [], 0
    for s in sizes:
        pos += int(rng.integers(1, gap_max + 1))
        off.append(pos)
        pos += int(s)
    return off, pos + int(rng.integers(1, gap_max + 1)) + TAIL


def _line_start(end, lo):
    """the first address >= end + 16 at block lo of a 128-byte line"""
    return end + 16 + (16 * lo - (end + 16)) % 128


def _lines(sizes):
    """offsets with record i at block i mod 8 of a line and 16..112 bytes between one range and the next in address
    order.  A range's end rules out at most two of the eight lo for its successor, so the address order is the index order
    with a record now and then taken a few places early: the lowest-numbered of the next records that fits, and a search
    over the orders of the last few."""
    n = len(sizes)
    off = [None] * n
    pool, end = list(range(n)), 0

    def fits(i, end, first):
        s = _line_start(end, i % 8)
        return s if first or s - end <= 112 else None

    def tail(pool, end, first):
        if not pool:
            return []
        for i in pool:
            s = fits(i, end, first)
            if s is not None:
                rest = tail([j for j in pool if j != i], s + sizes[i], False)
                if rest is not None:
                    return [(i, s)] + rest
        return None

    first = True
    while len(pool) > 12:
        i, s = next((i, s) for i in pool[:16] for s in [fits(i, end, first)] if s is not None)
        off[i], end, first = s, s + sizes[i], False
        pool.remove(i)
    placed = tail(pool, end, first)
    assert placed is not None, "no address order with 16..112-byte gaps"
    for i, s in placed:
        off[i], end = s, s + sizes[i]
    return off, (end + 64 + 15) // 16 * 16 + TAIL


def layout(name, shapes, in_place=False, seed=1):
    """the offsets of `shapes` in layout `name`.  In place the output's ranges (L + 16 bytes) serve input and output"""
    assert name in LAYOUTS
    lens = [s.L for s in shapes]
    outs = [L + 16 for L in lens]
    aads = [s.A for s in shapes]
    if name == "lines":
        out_off, out_size = _lines(outs)
        (in_off, in_size), (aad_off, aad_size) = _packed(lens, 16), _packed(aads, 16)
    elif name == "bytes":
        rng = np.random.default_rng(seed)
        (in_off, in_size), (out_off, out_size), (aad_off, aad_size) = (_place(rng, x, 64) for x in (lens, outs, aads))
    else:
        align = 16 if name == "packed16" else 1
        recs, in_size, out_size, aad_size = ptls_hip.layout_records(lens, aads, [s.key for s in shapes], [0] * len(shapes),
                                                                    align=align)
        in_off, out_off, aad_off = ([int(x) for x in recs[f]] for f in ("in_off", "out_off", "aad_off"))
        in_size, out_size, aad_size = in_size + TAIL, out_size + TAIL, aad_size + TAIL
    if in_place:
        in_off, in_size = out_off, out_size
    return Layout(tuple(in_off), tuple(out_off), tuple(aad_off), in_size, out_size, aad_size)


def descriptors(c, lay, seal=True):
    """RECORD_DTYPE descriptors of a seal over `lay`, or of the open that reads the seal's output buffer and writes the
    plaintexts at the seal's input offsets"""
    r = np.zeros(len(c.shapes), dtype=ptls_hip.RECORD_DTYPE)
    r["in_off"], r["out_off"] = (lay.in_off, lay.out_off) if seal else (lay.out_off, lay.in_off)
    r["aad_off"], r["seq"] = lay.aad_off, c.seqs
    r["len"], r["aad_len"], r["key"] = [s.L for s in c.shapes], [s.A for s in c.shapes], [s.key for s in c.shapes]
    if seal:
        r["flags"] = [0 if s.ctype is None else ptls_hip.record_tls13_type(s.ctype) for s in c.shapes]
    return r


# ---------------------------------------------------------------------------------------------------------------------
# images and their compare


def image(base, offs, pieces):
    """`base` with pieces[i] (bytes) laid in at offs[i]"""
    img = base.copy()
    for o, p in zip(offs, pieces):
        if len(p):
            assert o + len(p) <= len(img)
            img[o: o + len(p)] = np.frombuffer(p, np.uint8)
    return img


def covered(size, offs, sizes):
    """True at every byte that belongs to some record's range"""
    m = np.zeros(size, bool)
    for o, s in zip(offs, sizes):
        m[o: o + s] = True
    return m


Diff = namedtuple("Diff", "inside outside")  # positions (numpy arrays) of the differing bytes, by kind


def compare(got, want, offs, sizes):
    """the bytes of `got` that differ from the image `want`: inside a record's range / outside every record"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    bad = got != want
    own = covered(len(want), offs, sizes)
    return Diff(np.flatnonzero(bad & own), np.flatnonzero(bad & ~own))


def same(got, want, offs, sizes, what):
    d = compare(got, want, offs, sizes)
    assert d.inside.size == 0 and d.outside.size == 0, (
        f"{what}: {d.inside.size} bytes differ inside a record (first at {d.inside[:8].tolist()}), "
        f"{d.outside.size} outside every record (first at {d.outside[:8].tolist()}, "
        f"holding {[int(got[p]) for p in d.outside[:8]]})")


def mask_offsets(n):
    """masks 32 bytes apart at offset 8 (the stride32 layout of tests/test_gpu_copy_gaps.py)"""
    return [32 * i + 8 for i in range(n)], 32 * n + 16


def supp_entries(c, lay, oracle, hp_key, seed=5):
    """(SUPP_DTYPE entries, mask offsets and masks of the entries the device must serve, size of the mask buffer): every
    fifth entry disabled, some naming an hp_key outside the one-slot keyset, samples anywhere in ct || tag"""
    rng = np.random.default_rng(seed)
    n = len(c.shapes)
    mask_off, mask_size = mask_offsets(n)
    supp = np.zeros(n, dtype=ptls_hip.SUPP_DTYPE)
    moffs, masks = [], []
    for i, s in enumerate(c.shapes):
        off = s.L if i % 4 == 1 else int(rng.integers(0, s.L + 1))  # i % 4 == 1: the sample is the tag
        enabled = i % 5 != 2
        slot = 3 if i % 11 == 7 else 0  # 3: outside the keyset
        supp[i] = (lay.out_off[i] + off, mask_off[i], slot, ptls_hip.SUPP_ENABLE if enabled else 0)
        if enabled and slot == 0:
            moffs.append(mask_off[i])
            masks.append(oracle.aes_ecb(hp_key, c.sealed[i][off: off + 16]))
    return supp, moffs, masks, mask_size


# ---------------------------------------------------------------------------------------------------------------------
# the device run


def _cuda(arr):
    import torch
    t = torch.from_numpy(arr.view(np.uint8)).cuda()
    assert t.data_ptr() % 16 == 0  # the ALIGNED instantiations need aligned bases as well as aligned offsets
    return t


def mask_prefill(size):
    """position-dependent, so mask bytes that come back at a wrong offset differ as well (tests/test_gpu_copy_gaps.py)"""
    return ((7 + 131 * np.arange(size)) & 0xFF).astype(np.uint8)


Run = namedtuple("Run", "lay lanes out out_want inp inp_want aad aad_want mask mask_want mask_offs pt pt_want res")


def run(engine, oracle, c, layout_name, lanes, wg=0, in_place=False, supp=False):
    """one seal launch of the case `c` (then one open launch of what it wrote); every buffer after the launches and its
    expected image"""
    import torch
    lay = layout(layout_name, c.shapes, in_place=in_place)
    n = len(c.shapes)
    key_len = len(c.keys[0][0])
    rng = np.random.default_rng(77)
    ks = ptls_hip.KeySet(engine, key_len, len(c.keys))
    ks.set(0, b"".join(k for k, _ in c.keys), b"".join(iv for _, iv in c.keys))
    h_in = image(rng.integers(0, 256, lay.in_size, dtype=np.uint8), lay.in_off, c.inputs)
    h_aad = image(rng.integers(0, 256, lay.aad_size, dtype=np.uint8), lay.aad_off, c.aads)
    h_out = h_in if in_place else np.full(lay.out_size, FILL, np.uint8)
    d_in, d_aad = _cuda(h_in), _cuda(h_aad)
    d_out = d_in if in_place else _cuda(h_out)
    batch = ptls_hip.Batch(engine, descriptors(c, lay))
    batch.set_lanes(lanes)
    batch.set_workgroup(wg)
    assert batch.lanes == lanes
    mask = mask_want = mask_offs = None
    if supp:
        hp_key = oracle.stream(77, key_len)
        hp = ptls_hip.KeySet(engine, key_len, 1)
        hp.set(0, hp_key, None)
        entries, mask_offs, masks, mask_size = supp_entries(c, lay, oracle, hp_key)
        mbase = mask_prefill(mask_size)
        d_mask = _cuda(mbase.copy())
        batch.seal_supp(ks, hp, _cuda(entries), d_in, d_aad, d_out, d_mask)
        torch.cuda.synchronize()
        hp.close()
        mask, mask_want = d_mask.cpu().numpy(), image(mbase, mask_offs, masks)
    else:
        batch.seal(ks, d_in, d_aad, d_out)
        torch.cuda.synchronize()
    batch.close()
    out, out_want = d_out.cpu().numpy(), image(h_out, lay.out_off, c.sealed)
    inp, aad = d_in.cpu().numpy(), d_aad.cpu().numpy()
    # open what the launch wrote, the bytes between the records included, into a fresh buffer at the seal's input offsets
    pbase = np.full(lay.in_size, FILL, np.uint8)
    d_pt = _cuda(pbase.copy())
    d_res = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda")
    obatch = ptls_hip.Batch(engine, descriptors(c, lay, seal=False))
    obatch.set_lanes(lanes)
    obatch.set_workgroup(wg)
    obatch.open(ks, d_out, d_aad, d_pt, d_res)
    torch.cuda.synchronize()
    obatch.close()
    ks.close()
    res = [int(x) & UINT64_MAX for x in d_res.cpu().numpy().tolist()]
    return Run(lay, lanes, out, out_want, inp, out_want if in_place else h_in, aad, h_aad, mask, mask_want, mask_offs,
               d_pt.cpu().numpy(), image(pbase, lay.in_off, c.plains), res)


def check(engine, oracle, c, layout_name, lanes, **kw):
    r = run(engine, oracle, c, layout_name, lanes, **kw)
    lens = [s.L for s in c.shapes]
    outs = [L + 16 for L in lens]
    same(r.out, r.out_want, r.lay.out_off, outs, "seal output")
    same(r.inp, r.inp_want, r.lay.in_off, outs if kw.get("in_place") else lens, "seal input buffer")
    same(r.aad, r.aad_want, r.lay.aad_off, [s.A for s in c.shapes], "AAD buffer")
    if r.mask is not None:
        same(r.mask, r.mask_want, r.mask_offs, [16] * len(r.mask_offs), "header-protection masks")
    assert r.res == lens, [(i, x) for i, (x, L) in enumerate(zip(r.res, lens)) if x != L][:8]
    same(r.pt, r.pt_want, r.lay.in_off, lens, "open of the sealed image")
    return r


def main():
    lanes, key_len = int(sys.argv[1]), int(sys.argv[2])
    import torch
    # torch first: its HIP runtime must be the process's one before libptls_hip.so loads (as tests/dealing_case.py)
    assert torch.cuda.is_available()
    from oracle_lib import Oracle
    o = Oracle()
    eng = ptls_hip.Engine(0)
    c = case(o, key_len, lanes)
    r = run(eng, o, c, "lines", lanes, wg=768)
    eng.close()
    d = compare(r.out, r.out_want, r.lay.out_off, [s.L + 16 for s in c.shapes])
    behind = {off + s.L + 16 for off, s in zip(r.lay.out_off, c.shapes)}
    stray = set(d.outside.tolist())
    opened = int((r.pt != r.pt_want).sum()) + sum(1 for x, s in zip(r.res, c.shapes) if x != s.L)
    print(f"MISMATCHES records={len(c.shapes)} inside={d.inside.size} outside={d.outside.size} "
          f"behind_tag={len(stray & behind)} elsewhere={len(stray - behind)} "
          f"zeros={sum(1 for p in stray if r.out[p] == 0)} open={opened} "
          f"first={','.join(str(p) for p in d.outside[:4].tolist())} lib={ptls_hip.LIB_PATH}", flush=True)


if __name__ == "__main__":
    main()
