"""The layouts, shape lists and image compare of tests/seal_exact_case.py do what the GPU matrix relies on (no GPU needed).

A whole-buffer compare proves nothing if its layout leaves no fill where a stray store would land, if its shapes miss a
path of the kernel, or if its compare cannot tell a stray 0x00 from an untouched byte.
"""
import numpy as np
import pytest

import ptls_hip
import seal_exact_case as sx
from test_gpu_copy_gaps import mask_prefill

ALL_LANES = list(sx.BATCH_GS) + [sx.SPARSE_LANES]


def _ranges(offs, sizes):
    return sorted((o, o + s) for o, s in zip(offs, sizes))


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("lanes", ALL_LANES)
def test_lines_layout(lanes, in_place):
    shapes = sx.shapes_for(lanes)
    lay = sx.layout("lines", shapes, in_place=in_place)
    assert all(o % 16 == 0 for o in lay.in_off + lay.out_off + lay.aad_off)
    assert all((o >> 4) & 7 == i % 8 for i, o in enumerate(lay.out_off))
    rng = _ranges(lay.out_off, [s.L + 16 for s in shapes])
    gaps = [b[0] - a[1] for a, b in zip(rng, rng[1:])]
    assert min(gaps) >= 16 and max(gaps) <= 112, (min(gaps), max(gaps))
    assert rng[0][0] >= 16 and lay.out_size - rng[-1][1] >= 16  # fill before the first and behind the last record too
    for offs, sizes, size in ((lay.in_off, [s.L + (16 if in_place else 0) for s in shapes], lay.in_size),
                              (lay.aad_off, [s.A for s in shapes], lay.aad_size)):
        r = _ranges(offs, sizes)
        assert all(a[1] <= b[0] for a, b in zip(r, r[1:])) and r[-1][1] < size
    if in_place:
        assert (lay.in_off, lay.in_size) == (lay.out_off, lay.out_size)


@pytest.mark.parametrize("G", sx.BATCH_GS)
def test_lines_layout_meets_every_lo_at_every_k(G):
    shapes = sx.batch_shapes(G)
    lay = sx.layout("lines", shapes)
    for k in sx.batch_ks(G):
        for r in sx.RS:
            los = {(o >> 4) & 7 for o, s in zip(lay.out_off, shapes) if s.L == 16 * k + r}
            assert los == set(range(8)), (k, r, los)


@pytest.mark.parametrize("name", ["packed16", "bytes", "packed1"])
@pytest.mark.parametrize("lanes", [1, 32, 64])
def test_other_layouts(lanes, name):
    shapes = sx.shapes_for(lanes)
    for in_place in (False, True):
        lay = sx.layout(name, shapes, in_place=in_place)
        for offs, sizes, size in ((lay.in_off, [s.L + (16 if in_place else 0) for s in shapes], lay.in_size),
                                  (lay.out_off, [s.L + 16 for s in shapes], lay.out_size),
                                  (lay.aad_off, [s.A for s in shapes], lay.aad_size)):
            r = _ranges(offs, sizes)
            assert all(a[1] <= b[0] for a, b in zip(r, r[1:])) and r[-1][1] < size
        if name == "packed16":
            assert all(o % 16 == 0 for o in lay.in_off + lay.out_off + lay.aad_off)
        if name == "bytes":  # the unaligned instantiation, at every residue
            assert {o % 16 for o in lay.out_off} >= set(range(1, 16))
            assert {o % 16 for o in lay.in_off} >= set(range(1, 16))
            r = _ranges(lay.out_off, [s.L + 16 for s in shapes])
            assert all(1 <= b[0] - a[1] <= 64 for a, b in zip(r, r[1:]))
        if name == "packed1":
            r = _ranges(lay.out_off, [s.L + 16 for s in shapes])
            assert all(a[1] == b[0] for a, b in zip(r, r[1:]))


@pytest.mark.parametrize("G", sx.BATCH_GS)
def test_batch_shapes_cover_the_stretch(G):
    shapes = sx.batch_shapes(G)
    iters = {(s.L >> 4) // (sx.PURE_BLOCKS * G) for s in shapes}
    assert iters >= {0, 1, 2, 3}
    ks = set(sx.batch_ks(G))
    for m in (1, 2, 3):  # both sides of every iteration count: one block less, exactly, one block more
        assert {m * 2 * G, m * 2 * G + 1} <= ks
        assert any(k < m * 2 * G and k >= (m - 1) * 2 * G for k in ks)
    assert {4 * G - 1, 4 * G, 4 * G + 1} <= ks
    assert {s.L & 15 for s in shapes} == set(sx.RS)
    assert {s.A for s in shapes} == set(sx.batch_aads(G))
    for k in ks:  # k x r in full, eight records (one per lo) each
        for r in sx.RS:
            assert sum(1 for s in shapes if s.L == 16 * k + r) == 8
    keys = [s.key for s in shapes]
    assert keys == sorted(keys) and set(keys) == {0, 1}  # two key runs
    for key in (0, 1):
        assert {s.L >> 4 for s in shapes if s.key == key} == ks
    assert max(s.L for s in shapes) <= 16 * (6 * 32 + 1) + 15
    flagged = [i for i, s in enumerate(shapes) if s.ctype is not None]
    assert {shapes[i].ctype for i in flagged} == {21, 22, 23} and all(i % 7 == 3 for i in flagged)
    assert len(flagged) >= len(shapes) // 7 - 8  # every seventh, but for the records of no bytes


def test_sparse_shapes_cover_the_horner_steps():
    shapes = sx.sparse_shapes()
    ns = {sx.ghash_elements(s.L, s.A) for s in shapes}
    assert ns == set(sx.SPARSE_N)
    assert any(n <= 64 for n in ns) and 65 in ns and any(n > 128 for n in ns)
    for N in sx.SPARSE_N:
        if N >= 4:
            assert {(s.L & 15, s.A) for s in shapes if sx.ghash_elements(s.L, s.A) == N} == \
                {(r, A) for r in sx.RS for A in sx.SPARSE_AADS}
    assert [s.key for s in shapes] == list(range(len(shapes)))  # a key per record
    lay = sx.layout("lines", shapes)
    for L, A in {(s.L, s.A) for s in shapes}:  # the repeats put every shape at several lo
        assert len({(o >> 4) & 7 for o, s in zip(lay.out_off, shapes) if (s.L, s.A) == (L, A)}) >= 3


def test_compare_sees_stray_wrong_and_zero_bytes():
    offs, pieces = [16, 80], [b"\x01" * 21, b"\x02" * 32]
    sizes = [len(p) for p in pieces]
    base = np.full(160, sx.FILL, np.uint8)
    want = sx.image(base, offs, pieces)
    got = want.copy()
    sx.same(got, want, offs, sizes, "exact")
    got[50] ^= 0x4B  # a stray byte between the records
    d = sx.compare(got, want, offs, sizes)
    assert (d.inside.tolist(), d.outside.tolist()) == ([], [50])
    with pytest.raises(AssertionError, match=r"0 bytes differ inside a record .*1 outside every record \(first at \[50\]"):
        sx.same(got, want, offs, sizes, "stray")
    got = want.copy()
    got[90] ^= 1  # a wrong byte inside the second record
    d = sx.compare(got, want, offs, sizes)
    assert (d.inside.tolist(), d.outside.tolist()) == ([90], [])
    with pytest.raises(AssertionError, match=r"1 bytes differ inside a record \(first at \[90\]\), 0 outside"):
        sx.same(got, want, offs, sizes, "wrong")
    got = want.copy()
    got[16 + 21] = 0  # a stray 0x00 right behind the first record
    d = sx.compare(got, want, offs, sizes)
    assert (d.inside.tolist(), d.outside.tolist()) == ([], [37])
    # ... which a zero-filled buffer, as the record-by-record seal tests use, cannot show
    zwant = sx.image(np.zeros(160, np.uint8), offs, pieces)
    zgot = zwant.copy()
    zgot[16 + 21] = 0
    d = sx.compare(zgot, zwant, offs, sizes)
    assert d.inside.size == 0 and d.outside.size == 0 and np.array_equal(zgot, zwant)
    # the masks' prefill has no constant byte to hide behind either
    m = sx.mask_prefill(96)
    assert np.array_equal(m, mask_prefill(96)) and len(set(m[:64].tolist())) == 64


def test_flagged_records_expect_the_type_byte_not_the_input(oracle):
    c = sx.case(oracle, 16, 4)
    flagged = [i for i, s in enumerate(c.shapes) if s.ctype is not None]
    assert flagged
    for i in flagged:
        s = c.shapes[i]
        assert c.inputs[i][-1] == sx.POISON and c.inputs[i][:-1] == c.plains[i][:-1]
        assert c.plains[i][-1] == s.ctype != sx.POISON
        assert c.sealed[i] == oracle.seal(*c.keys[s.key], c.seqs[i], c.aads[i], c.inputs[i][:-1] + bytes([s.ctype]))
        assert c.sealed[i] != oracle.seal(*c.keys[s.key], c.seqs[i], c.aads[i], c.inputs[i])
    for i, s in enumerate(c.shapes):
        if s.ctype is None:
            assert c.inputs[i] == c.plains[i]
        assert len(c.sealed[i]) == s.L + 16
    d = sx.descriptors(c, sx.layout("lines", c.shapes))
    assert [int(f) for f in d["flags"]] == [0 if s.ctype is None else ptls_hip.record_tls13_type(s.ctype) for s in c.shapes]
    assert not sx.descriptors(c, sx.layout("lines", c.shapes), seal=False)["flags"].any()


def test_supp_entries(oracle):
    c = sx.case(oracle, 16, 4)
    lay = sx.layout("bytes", c.shapes)
    hp_key = oracle.stream(77, 16)
    supp, moffs, masks, size = sx.supp_entries(c, lay, oracle, hp_key)
    n = len(c.shapes)
    assert [int(x) for x in supp["mask_off"]] == [32 * i + 8 for i in range(n)] and size == 32 * n + 16
    off = [int(supp["sample_off"][i]) - lay.out_off[i] for i in range(n)]
    assert all(0 <= o <= s.L for o, s in zip(off, c.shapes))
    assert any(o == s.L for o, s in zip(off, c.shapes)) and any(0 < s.L - o < 16 for o, s in zip(off, c.shapes))
    disabled = [i for i in range(n) if not supp["flags"][i] & ptls_hip.SUPP_ENABLE]
    assert disabled == list(range(2, n, 5))
    outside = [i for i in range(n) if supp["hp_key"][i] != 0]
    assert outside and all(supp["hp_key"][i] >= 1 for i in outside)
    served = [i for i in range(n) if i not in disabled and i not in outside]
    assert moffs == [32 * i + 8 for i in served] and len(masks) == len(served)
    i = served[3]
    assert masks[3] == oracle.aes_ecb(hp_key, c.sealed[i][off[i]: off[i] + 16])
