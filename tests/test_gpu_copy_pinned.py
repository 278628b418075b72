"""The COPY host transport on PINNED caller buffers: exactly the records' bytes and exactly the records' masks.

With pageable buffers (tests/test_gpu_copy_gaps.py) HIP's copies block the host, so the pipeline's three slot streams run
one slice after another.  With page-locked buffers and ptls_hip_pipeline_set_transport(p, PTLS_HIP_TRANSPORT_COPY), a
choice INTEGRATION.md offers, the slices' uploads, kernels and copies back really overlap, and whatever one slice writes
into the caller's buffers outside its own records races with the other slices.  The header-protection masks are the point:
a slice used to upload and copy back its whole mask span, so with masks of different slices interleaved in h_mask a
slice's copy back overwrote the masks another slice had just delivered with the stale bytes it had uploaded before.

The same helpers as the pageable cases, on torch.empty(size).pin_memory() buffers: one pipeline runs open, seal,
seal_supp, open, seal with 1-byte gaps; seal_supp with three mask layouts (mask_offsets: in record order with spare
bytes, permuted over the whole buffer, permuted and packed) for descriptors in output order (the copy transport's in_order
path) and shuffled; TLS 1.3 seal and open.  Every WHOLE output and mask buffer equals its expected image (the prefill,
position-dependent for masks, with the CPU oracle's records and oracle.aes_ecb(hp_key, sample) laid in), bit for bit, on
the copy transport and, as the control, on the mapped transport with the same buffers.  One call per case: the layouts
make a stale copy back land whenever two slices overlap at all.

Last, the copy transport's refusals that the public API can reach, each followed by a correct call on the same pipeline
(a refused call drains the slots and must leave the pipeline usable), and the layouts that were refused before masks
travelled compact: masks spanning more than a slice, and more masks than a slice's mask staging holds.
"""
import numpy as np
import pytest

import ptls_hip
from test_gpu_copy_gaps import MASK_LAYOUTS, Case, _open, _order, _seal, _seal_supp, _tls13

pytestmark = pytest.mark.gpu
TRANSPORTS = {"copy": ptls_hip.TRANSPORT_COPY, "mapped": ptls_hip.TRANSPORT_MAPPED}
N_MANY = 400


@pytest.fixture(scope="module")
def cases(engine, oracle):
    """the CPU oracle's seals of a Case, computed once per (key size, record count) and shared by every slice size,
    order, layout and transport; the layouts of a test come from a generator seeded by that test"""
    cache = {}

    def get(bits, n, seed):
        if (bits, n) not in cache:
            cache[bits, n] = Case(engine, oracle, bits, n, seed=1000 + bits + n)
        cache[bits, n].rng = np.random.default_rng(seed)
        return cache[bits, n]

    yield get
    for c in cache.values():
        c.ks.close()


def _check_slices(case, slice_kib):
    """a lower bound of the slice count that follows from the layout (the pipeline does not report its count): a slice's
    output span fits slice_bytes, so the smallest output of the sequence (the plaintexts of open) needs at least
    ceil(bytes / slice_bytes) slices.  400 records at 64 KiB: six or more, twice the pipeline's three slots"""
    if len(case.lens) == N_MANY and slice_kib == 64:
        assert -(-sum(case.lens) // (slice_kib << 10)) >= 6, "the length mix no longer fills six 64 KiB slices"


@pytest.mark.parametrize("transport", ["copy", "mapped"])
@pytest.mark.parametrize("order", ["in_order", "shuffled"])
@pytest.mark.parametrize("n", [N_MANY, 5])
@pytest.mark.parametrize("slice_kib", [64, 1024])
@pytest.mark.parametrize("bits", [128, 256])
def test_pinned_buffers_receive_only_record_bytes(engine, oracle, cases, bits, slice_kib, n, order, transport):
    case = cases(bits, n, seed=bits + slice_kib + n)
    _check_slices(case, slice_kib)
    perm = _order(n, order == "shuffled", case.rng)
    tr = TRANSPORTS[transport]
    pipe = ptls_hip.Pipeline(engine, slice_kib << 10, transport=tr)
    _open(case, pipe, 64, perm, "pinned", tr)  # first: the staging now holds plaintext
    _seal(case, pipe, 64, perm, "pinned", tr)
    _seal_supp(case, pipe, oracle, 64, perm, "pinned", tr)
    _open(case, pipe, 64, perm, "pinned", tr)
    _seal(case, pipe, 1, perm, "pinned", tr)  # 1-byte gaps
    pipe.close()


@pytest.mark.parametrize("transport", ["copy", "mapped"])
@pytest.mark.parametrize("layout", MASK_LAYOUTS)
@pytest.mark.parametrize("order", ["in_order", "shuffled"])
@pytest.mark.parametrize("n", [N_MANY, 5])
@pytest.mark.parametrize("slice_kib", [64, 1024])
@pytest.mark.parametrize("bits", [128, 256])
def test_pinned_masks_are_exact(engine, oracle, cases, bits, slice_kib, n, order, layout, transport):
    """every enabled entry with a valid hp_key has its record's mask at mask_off; every other byte of h_mask, the
    masks of disabled entries and of entries naming an hp_key outside the keyset included, keeps its prefill"""
    case = cases(bits, n, seed=bits + slice_kib + n + 7)
    _check_slices(case, slice_kib)
    if n == N_MANY:  # no slice's mask span can reach slice_bytes / 4, whatever the permutation
        assert 32 * n + 16 <= (64 << 10) // 4
    perm = _order(n, order == "shuffled", case.rng)
    tr = TRANSPORTS[transport]
    pipe = ptls_hip.Pipeline(engine, slice_kib << 10, transport=tr)
    _seal_supp(case, pipe, oracle, 64, perm, "pinned", tr, layout)
    pipe.close()


@pytest.mark.parametrize("transport", ["copy", "mapped"])
@pytest.mark.parametrize("slice_kib", [64, 1024])
def test_pinned_tls13_seal_and_open_gaps_between_messages(engine, oracle, slice_kib, transport):
    _tls13(engine, oracle, slice_kib, "pinned", TRANSPORTS[transport])


# ---- the copy transport's refusals ---------------------------------------------------------------------------------------

SMALL = [100, 3000, 16, 0, 1350]


def _copy_pipe(engine):
    return ptls_hip.Pipeline(engine, 64 << 10, transport=ptls_hip.TRANSPORT_COPY)


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
def test_copy_refuses_a_record_larger_than_a_slice(engine, oracle, kind):
    big = Case(engine, oracle, 128, 3, seed=1, lens=[100, (64 << 10) + 1, 16])
    good = Case(engine, oracle, 128, 5, seed=2, lens=SMALL)
    pipe = _copy_pipe(engine)
    with pytest.raises(ptls_hip.HipError, match=r"record 1 does not fit a 65536-byte slice"):
        _seal(big, pipe, 8, np.arange(3), kind)
    with pytest.raises(ptls_hip.HipError, match=r"record 1 does not fit a 65536-byte slice"):
        _open(big, pipe, 8, np.arange(3), kind)
    _seal(good, pipe, 8, np.arange(5), kind)
    _open(good, pipe, 8, np.arange(5), kind)
    pipe.close()
    big.ks.close()
    good.ks.close()


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
def test_copy_refuses_a_sample_outside_the_slice_output(engine, oracle, kind):
    """records 0 | 1, 2 make two 64 KiB slices; record 0's sample lies in record 1's output, which its slice does not stage"""
    case = Case(engine, oracle, 128, 3, seed=3, lens=[40000, 40000, 100])
    pipe = _copy_pipe(engine)

    def far_sample(supp, out_off):
        supp[0]["sample_off"] = out_off[1] + 8

    with pytest.raises(ptls_hip.HipError, match=r"sample of record 0 is outside the slice's output"):
        _seal_supp(case, pipe, oracle, 8, np.arange(3), kind, edit=far_sample)
    _seal_supp(case, pipe, oracle, 8, np.arange(3), kind)
    pipe.close()
    case.ks.close()


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
def test_copy_refusal_in_a_later_slice_drops_the_undelivered_masks(engine, oracle, kind):
    """the same two slices, refused while the SECOND is planned (record 1's sample lies in record 0's output): slice 0 is
    in flight with record 0's mask still to be placed.  The refused call drains it; the correct call on the same pipeline
    must not deliver that mask as well, nor put its own masks after it"""
    case = Case(engine, oracle, 128, 3, seed=6, lens=[40000, 40000, 100])
    pipe = _copy_pipe(engine)

    def early_sample(supp, out_off):
        assert supp[0]["flags"] & ptls_hip.SUPP_ENABLE and supp[0]["hp_key"] == 0  # slice 0 carries a mask
        supp[1]["sample_off"] = out_off[0] + 8

    with pytest.raises(ptls_hip.HipError, match=r"sample of record 1 is outside the slice's output"):
        _seal_supp(case, pipe, oracle, 8, np.arange(3), kind, layout="perm16", edit=early_sample)
    _seal_supp(case, pipe, oracle, 8, np.arange(3), kind, layout="stride32")
    pipe.close()
    case.ks.close()


@pytest.mark.parametrize("order", ["in_order", "shuffled"])
@pytest.mark.parametrize("kind", ["pageable", "pinned"])
def test_copy_masks_may_span_more_than_a_slice(engine, oracle, kind, order):
    """five records of one slice with masks 20 000 bytes apart (80 KB from the first to the last, more than the 64 KiB
    slice and than the slice_bytes / 4 a slice's mask span was once limited to): served, and exact"""
    case = Case(engine, oracle, 256, 5, seed=4, lens=SMALL)
    perm = _order(5, order == "shuffled", case.rng)
    pipe = _copy_pipe(engine)
    _seal_supp(case, pipe, oracle, 8, perm, kind, layout="far")
    _seal_supp(case, pipe, oracle, 8, perm, kind, layout="perm16")
    pipe.close()
    case.ks.close()


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
def test_copy_more_masks_than_a_slice_stages(engine, oracle, kind):
    """1600 records of 8 bytes without AAD fit one 64 KiB slice by their bytes (outputs 25 bytes apart, AAD offsets at
    most 8 apart against the slice_bytes / 4 of AAD staging), but a slice stages at most slice_bytes / 64 = 1024 masks:
    the slice ends there and the next one takes the rest"""
    n = 1600
    case = Case(engine, oracle, 128, n, seed=5, lens=[8] * n, aad_len=0)
    assert sum(1 for i in range(n) if i % 5 != 2 and i % 11 != 7) > (64 << 10) // 64
    assert 25 * n + 1 <= 64 << 10 and 8 * n + 8 <= (64 << 10) // 4
    pipe = _copy_pipe(engine)
    _seal_supp(case, pipe, oracle, 1, np.arange(n), kind, layout="perm16")
    pipe.close()
    case.ks.close()
