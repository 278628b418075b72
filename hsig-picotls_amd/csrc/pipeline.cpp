/*
 * pipeline.cpp -- host-resident records (north_star: TLS records start and end in socket buffers).  A pipeline moves
 * slices of a record list through the batch kernels either by letting the kernels read and write the caller's pinned host
 * buffers over PCIe (MAPPED) or by staging through device buffers with the copy engines (COPY).
 */
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host.h"
/* ---------------------------------------------------------------------------------------------- */
/* host-resident pipeline: pinned H2D -> kernel -> D2H, overlapped over NSLOT streams                */
/* ---------------------------------------------------------------------------------------------- */

static const int NSLOT = 3;

struct PipeSlot {
    hipStream_t stream;
    hipEvent_t done;
    uint8_t *d_in, *d_out, *d_aad, *d_mask;
    ptls_hip_record_t *d_recs, *d_recs_ord;
    Chunk *d_chunks;
    uint32_t *d_order;
    uint64_t *d_result;
    ptls_hip_supp_t *d_supp;
    /* pinned host staging for the slice's descriptors / chunks / record order / header-protection descriptors */
    ptls_hip_record_t *h_recs, *h_recs_ord;
    Chunk *h_chunks;
    uint32_t *h_order;
    ptls_hip_supp_t *h_supp;
    /* copy transport, allocated on a slice with gaps between its records: the caller's bytes of those gaps (packed) and
     * where they go in d_out, pinned and on the device */
    uint8_t *h_gap, *d_gap;
    GapPiece *h_gapd, *d_gapd;
    /* copy transport, allocated on a slice with header protection: the slice's masks arrive here, packed, by one copy;
     * mask t goes to mask_host + mask_dst[t] once the slice is done (slot_wait) */
    uint8_t *h_mask;
    uint8_t *mask_host;
    std::vector<uint64_t> mask_dst;
    /* QUIC packets, allocated on the slot's first slice of them (slot_quic_buffers): the slice-local packet descriptors,
     * pinned and on the device; open: the packet numbers when they cannot go straight to the caller's mapped array, and on
     * the copy transport the packed header entries (quic_slice_kernel.hip), which arrive in h_hdr by one copy; entry t goes
     * to hdr_host + hdr_dst[t] once the slice is done (slot_wait) */
    ptls_hip_quic_packet_t *h_pkts, *d_pkts;
    uint64_t *d_pn;
    uint8_t *d_hdr, *h_hdr;
    uint8_t *hdr_host;
    std::vector<HdrDst> hdr_dst;
    bool busy;
};

struct st_ptls_hip_pipeline_t {
    ptls_hip_engine_t *eng;
    size_t slice_bytes, max_recs;
    int transport;      /* PTLS_HIP_TRANSPORT_*: what the caller asked for */
    int last_transport; /* what the last seal/open used */
    int algo;           /* PTLS_HIP_ALGO_*: the keysets the pipeline serves */
    int chacha_lanes;   /* ChaCha pipelines: 0 = from the slice's records, or the forced width (1, 4, 16, 64) */
    int chacha_layout;  /* ... and PTLS_HIP_CHACHA_LAYOUT_* */
    PipeSlot slot[NSLOT];
    /* scratch of launch_slice alone: the chunks and the order of the AES-GCM slice it is planning */
    std::vector<Chunk> ch;
    std::vector<uint32_t> order;
};

/* a slot's fixed buffers, for ptls_hip_pipeline_new and _free: f(&pointer, bytes, pinned host memory or device memory).
 * The launch plan's buffers (chunks, record order) exist on AES-GCM pipelines only: the ChaCha kernels take the records in
 * descriptor order. */
template <class F> static void slot_buffers(PipeSlot &s, size_t slice_bytes, size_t max_recs, bool plan, F f)
{
    f(&s.d_in, slice_bytes + 64, false);
    f(&s.d_out, slice_bytes + 64, false);
    f(&s.d_aad, slice_bytes / 4 + 64, false);
    f(&s.d_mask, slice_bytes / 4 + 64, false);
    f(&s.d_supp, max_recs * sizeof(ptls_hip_supp_t), false);
    f(&s.h_supp, max_recs * sizeof(ptls_hip_supp_t), true);
    f(&s.d_recs, max_recs * sizeof(ptls_hip_record_t), false);
    if (plan) {
        f(&s.d_recs_ord, max_recs * sizeof(ptls_hip_record_t), false);
        f(&s.h_recs_ord, max_recs * sizeof(ptls_hip_record_t), true);
        f(&s.d_chunks, max_recs * sizeof(Chunk), false);
        f(&s.d_order, max_recs * sizeof(uint32_t), false);
        f(&s.h_order, max_recs * sizeof(uint32_t), true);
    }
    f(&s.d_result, max_recs * sizeof(uint64_t), false);
    f(&s.h_recs, max_recs * sizeof(ptls_hip_record_t), true);
    if (plan)
        f(&s.h_chunks, max_recs * sizeof(Chunk), true);
}

extern "C" ptls_hip_pipeline_t *ptls_hip_pipeline_new(ptls_hip_engine_t *eng, size_t slice_bytes)
{
    return ptls_hip_pipeline_new_algo(eng, PTLS_HIP_ALGO_AESGCM, slice_bytes);
}

extern "C" ptls_hip_pipeline_t *ptls_hip_pipeline_new_algo(ptls_hip_engine_t *eng, int algo, size_t slice_bytes)
{
    if (eng == nullptr || slice_bytes < (1u << 16) || !(algo == PTLS_HIP_ALGO_AESGCM || algo == PTLS_HIP_ALGO_CHACHA20POLY1305)) {
        fail(PTLS_HIP_EINVAL, "pipeline_new: bad arguments");
        return nullptr;
    }
    DeviceGuard g(eng->device);
    auto *p = new st_ptls_hip_pipeline_t();
    p->eng = eng;
    p->algo = algo;
    p->slice_bytes = slice_bytes;
    p->max_recs = slice_bytes / 16 + 1;
    bool ok = true;
    for (auto &s : p->slot) {
        ok = ok && hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&s.done, hipEventDisableTiming) == hipSuccess;
        slot_buffers(s, slice_bytes, p->max_recs, algo == PTLS_HIP_ALGO_AESGCM, [&ok](auto **pp, size_t bytes, bool pinned) {
            ok = ok && (pinned ? hipHostMalloc(pp, bytes, hipHostMallocDefault) : hipMalloc(pp, bytes)) == hipSuccess;
        });
        s.busy = false;
    }
    if (!ok) {
        fail(PTLS_HIP_ENOMEM, "pipeline_new: cannot allocate %d x %zu bytes of staging", NSLOT, slice_bytes);
        ptls_hip_pipeline_free(p);
        return nullptr;
    }
    return p;
}

extern "C" void ptls_hip_pipeline_free(ptls_hip_pipeline_t *p)
{
    if (p == nullptr)
        return;
    DeviceGuard g(p->eng->device);
    for (auto &s : p->slot) {
        if (s.stream != nullptr)
            (void)hipStreamSynchronize(s.stream);
        slot_buffers(s, p->slice_bytes, p->max_recs, p->algo == PTLS_HIP_ALGO_AESGCM,
                     [](auto **pp, size_t, bool pinned) { (void)(pinned ? hipHostFree(*pp) : hipFree(*pp)); });
        /* the copy transport's lazy staging (slot_gap_buffers, slot_mask_buffer) */
        (void)hipHostFree(s.h_gap);
        (void)hipFree(s.d_gap);
        (void)hipHostFree(s.h_gapd);
        (void)hipFree(s.d_gapd);
        (void)hipHostFree(s.h_mask);
        (void)hipHostFree(s.h_pkts);
        (void)hipFree(s.d_pkts);
        (void)hipFree(s.d_pn);
        (void)hipFree(s.d_hdr);
        (void)hipHostFree(s.h_hdr);
        if (s.done != nullptr)
            (void)hipEventDestroy(s.done);
        if (s.stream != nullptr)
            (void)hipStreamDestroy(s.stream);
    }
    delete p;
}

extern "C" int ptls_hip_pipeline_set_transport(ptls_hip_pipeline_t *p, int transport)
{
    if (p == nullptr ||
        !(transport == PTLS_HIP_TRANSPORT_AUTO || transport == PTLS_HIP_TRANSPORT_COPY || transport == PTLS_HIP_TRANSPORT_MAPPED))
        return fail(PTLS_HIP_EINVAL, "pipeline_set_transport: bad arguments");
    p->transport = transport;
    return 0;
}

extern "C" int ptls_hip_pipeline_last_transport(ptls_hip_pipeline_t *p)
{
    return p->last_transport;
}

extern "C" int ptls_hip_pipeline_algo(ptls_hip_pipeline_t *p)
{
    return p != nullptr ? p->algo : fail(PTLS_HIP_EINVAL, "pipeline_algo: null pipeline");
}

extern "C" int ptls_hip_pipeline_set_chacha_lanes(ptls_hip_pipeline_t *p, int lanes, int layout)
{
    if (p == nullptr || p->algo != PTLS_HIP_ALGO_CHACHA20POLY1305)
        return fail(PTLS_HIP_EINVAL, "pipeline_set_chacha_lanes: not a ChaCha20-Poly1305 pipeline");
    if (!(lanes == 0 || lanes == 1 || lanes == 4 || lanes == 16 || lanes == 64) ||
        !(layout == PTLS_HIP_CHACHA_LAYOUT_AUTO || layout == PTLS_HIP_CHACHA_LAYOUT_BLOCKS || layout == PTLS_HIP_CHACHA_LAYOUT_RUNS) ||
        (layout == PTLS_HIP_CHACHA_LAYOUT_RUNS && lanes == 1))
        return fail(PTLS_HIP_EINVAL, "pipeline_set_chacha_lanes: lanes must be 0, 1, 4, 16 or 64 and layout a "
                                     "PTLS_HIP_CHACHA_LAYOUT_* (RUNS: 4 lanes or more)");
    p->chacha_lanes = lanes;
    p->chacha_layout = layout;
    return 0;
}

extern "C" int ptls_hip_host_register(void *ptr, size_t len)
{
    HIP_TRY(hipHostRegister(ptr, len, hipHostRegisterDefault), PTLS_HIP_ENODEV);
    return 0;
}

extern "C" int ptls_hip_host_unregister(void *ptr)
{
    HIP_TRY(hipHostUnregister(ptr), PTLS_HIP_ENODEV);
    return 0;
}

/* the device address of pinned (hipHostMalloc'd) or registered host memory, or nullptr if it is not mapped */
static void *mapped_ptr(const void *h)
{
    if (h == nullptr)
        return nullptr;
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<void *>(h), 0) != hipSuccess) {
        (void)hipGetLastError(); /* not an error of the pipeline: the copy transport is used */
        return nullptr;
    }
    return d;
}

/* the device address of h when pinned or registered host memory covers ALL of [h, h + need) with one mapping, else
 * nullptr; *partial = the start is mapped but not the whole span.  Such a buffer (registered only in part) must not
 * be handed to the kernels, which would touch unmapped host pages over PCIe, and the copy engines refuse it as well
 * (hipMemcpyAsync: invalid argument), so the call fails with EINVAL.  The mapping's range comes from the pointer
 * attributes; the last byte must also map, contiguously with the first. */
static void *mapped_span(const void *h, uint64_t need, bool *partial)
{
    void *d = mapped_ptr(h);
    if (d == nullptr || need <= 1)
        return d;
    const uintptr_t dp = reinterpret_cast<uintptr_t>(d);
    /* the allocation's range, queried and compared in the device address space: a span inside it is
     * mapped; otherwise the mapping of the span's last byte decides (one registration covering both ends) */
    uintptr_t start = 0;
    size_t size = 0;
    if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, reinterpret_cast<hipDeviceptr_t>(d)) == hipSuccess &&
        hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, reinterpret_cast<hipDeviceptr_t>(d)) == hipSuccess &&
        size != 0 && start <= dp && dp + need <= start + size)
        return d;
    (void)hipGetLastError();
    void *d_last = mapped_ptr(static_cast<const uint8_t *>(h) + (need - 1));
    if (d_last == nullptr || reinterpret_cast<uintptr_t>(d_last) != dp + (need - 1)) {
        *partial = true;
        return nullptr;
    }
    return d;
}

/* the refusal of a call that mapped_span found such a buffer in */
static int refuse_partial()
{
    return fail(PTLS_HIP_EINVAL, "pipeline: a host buffer is pinned or registered only in part (its mapping ends before "
                                 "the last byte the records touch): neither transport can use it");
}

/* lanes per record when the kernel reads and writes host memory: the launch is PCIe-bound, not LDS-bound, and wider
 * lane groups turn each load / store instruction into longer contiguous runs per record, i.e. fewer, larger PCIe
 * requests.  Measured (tools/hostmem_probe.py, seal+open GiB/s at 4 / 8 / 16 / 32 lanes): 1350-B records 31.7 /
 * 34.8 / 36.7 / 39.5; 16-KiB records - / 36.6 / 40.2 / 41.5; 64 B - 16 KiB over 64K keys at 16 / 32: 28.6 / 36.2.
 * Records of >= 64 GHASH elements go to the wave-per-record kernel (one 1-KiB run per wave instruction): 16 / 32 / 64
 * lanes 1350-B records 36.5 / 39.2 / 40.4, 16-KiB records 40.1 / 41.5 / 42.7 (one 1-GiB batch each).
 * Batches for the sparse-key kernel keep it. */
static int mapped_lanes(const ptls_hip_record_t *recs, size_t n, unsigned ncu)
{
    const int lanes = choose_lanes(recs, n, ncu);
    if (lanes == SPARSE_LANES || n == 0)
        return lanes;
    double sum = 0;
    for (size_t i = 0; i < n; ++i)
        sum += (double)((recs[i].aad_len + 15) / 16 + (recs[i].len + 15) / 16 + 1);
    const double mean = sum / (double)n;
    return mean >= 64 ? SPARSE_LANES : mean >= 32 ? 32 : mean >= 16 ? std::max(lanes, 16) : lanes;
}

/* the record kernel of a ChaCha slice: lanes per record, and whether the runs kernel (chacha_runs_kernel.hip: one
 * contiguous run of 16 x lanes bytes per group and instruction) or chacha_kernel.hip's (a lane per 64-byte block) */
struct ChaChaPlan {
    int lanes;
    bool runs;
};

/* ... when the kernel reads and writes host memory.  As for AES the launch is PCIe-bound and the width decides, more than
 * the layout does: a wide group of the block kernel touches the same contiguous span with its four instructions together.
 * Measured (tools/bench_chacha_host.py, profiles/chacha_host_bench.log: 1 GiB in pinned memory, seal+open GiB/s, medians of
 * three rounds of five steps, block kernel / runs kernel at 4, 16, 64 lanes; AES-128-GCM mapped in the same run beside it):
 *   65 536 x 16 KiB, one key    36.3 / 34.4   38.0 / 38.1   39.9 / 41.3   AES 40.8
 *   1 350 B over 65 536 keys    30.5 / 29.1   33.9 / 32.4   35.0 / 35.0   AES 35.0
 *   256 B over 65 536 keys      21.9 / 20.5   22.4 / 22.6   20.1 / 19.6   AES 18.8
 * (step-to-step spread mostly below 0.3, single steps up to 1.5 lower.)  The runs kernel wins only where every trip is full,
 * 64 lanes on records of 64 blocks or more (+1.4, above the spread); at 1 350 B (21 blocks) the two tie at 64 lanes and the
 * block kernel is ahead at 16 and 4; 64 lanes lose to 16 once a record has only four blocks.  So: records of 64 whole blocks
 * or more in the mean take the runs kernel at 64 lanes, of 16 or more the block kernel at 64, shorter ones the block kernel
 * at 16.  (Between 21 and 256 blocks, and below 4, nothing was measured: 64 is where a runs trip has no empty place.) */
static ChaChaPlan mapped_chacha_lanes(const ptls_hip_record_t *recs, size_t n)
{
    double sum = 0;
    for (size_t i = 0; i < n; ++i)
        sum += (double)(recs[i].len / 64);
    const double blocks = n != 0 ? sum / (double)n : 0;
    return blocks >= 64 ? ChaChaPlan{64, true} : blocks >= 16 ? ChaChaPlan{64, false} : ChaChaPlan{16, false};
}

/* The copy transport's staging is device memory: the block kernel at the width of the device-resident calls.
 * ptls_hip_pipeline_set_chacha_lanes overrides the width, the layout or both, on both transports; the runs kernel needs 4
 * lanes, so a forced width of 1 keeps the block kernel and a forced RUNS widens an automatic 1 to 4. */
static ChaChaPlan chacha_plan(const ptls_hip_pipeline_t *p, const ptls_hip_record_t *recs, size_t n, bool mapped)
{
    ChaChaPlan c = mapped ? mapped_chacha_lanes(recs, n) : ChaChaPlan{choose_chacha_lanes(recs, n, (unsigned)p->eng->ncu), false};
    if (p->chacha_layout != PTLS_HIP_CHACHA_LAYOUT_AUTO)
        c.runs = p->chacha_layout == PTLS_HIP_CHACHA_LAYOUT_RUNS;
    if (p->chacha_lanes != 0)
        c.lanes = p->chacha_lanes;
    else if (c.runs && c.lanes < 4)
        c.lanes = 4;
    c.runs = c.runs && c.lanes >= 4;
    return c;
}

/* wait for the slot's slice and deliver its masks (copy transport: the slice's masks arrived packed in s.h_mask) and the
 * unprotected header bytes of its QUIC packets (copy transport, open: packed in s.h_hdr, quic_slice_kernel.hip).
 * Pinned buffers make slices overlap: while these header bytes are placed in h_pkt, a later slice's upload may be reading a
 * span of h_pkt that contains them (descriptors not in h_pkt order).  That is harmless: the bytes belong to no packet of
 * that slice, so nothing reads them from its staging, and nothing of its staging's span is copied back to h_pkt. */
static int slot_wait(PipeSlot &s)
{
    if (!s.busy)
        return 0;
    HIP_TRY(hipEventSynchronize(s.done), PTLS_HIP_ENODEV);
    for (size_t t = 0; t < s.mask_dst.size(); ++t)
        std::memcpy(s.mask_host + s.mask_dst[t], s.h_mask + 16 * t, 16);
    s.mask_dst.clear();
    for (size_t t = 0; t < s.hdr_dst.size(); ++t) {
        const uint8_t *e = s.h_hdr + 8 * t;
        if (e[0] == 0) /* PTLS_HIP_QUIC_UNPROTECTED: nothing is written */
            continue;
        uint8_t *hdr = s.hdr_host + s.hdr_dst[t].off;
        hdr[0] = e[1];
        std::memcpy(hdr + s.hdr_dst[t].pn_offset, e + 2, (size_t)e[0] - 1);
    }
    s.hdr_dst.clear();
    s.busy = false;
    return 0;
}

/* the slice on s.stream is complete when s.done is: slot_wait */
static int slot_submit(PipeSlot &s)
{
    HIP_TRY(hipEventRecord(s.done, s.stream), PTLS_HIP_ENODEV);
    s.busy = true;
    return 0;
}

/* wait for every slice still in flight and free the slots on an error path: an earlier slice's kernel or copy may still
 * read or write the caller's host buffers, which the caller may release once the call returned.  Every stream is waited
 * for, not only those of busy slots: the slice that failed may have queued copies from the caller's buffers already. */
static void drain_slots(ptls_hip_pipeline_t *p)
{
    for (auto &s : p->slot) {
        (void)hipStreamSynchronize(s.stream);
        s.busy = false;
        s.mask_dst.clear(); /* the call failed: masks that were not delivered yet are not delivered */
        s.hdr_dst.clear();  /* ... nor are header bytes */
    }
}

/* One slice on slot s, the same for both transports and both algorithms, once its slice-local descriptors sit in s.h_recs
 * (and s.h_supp): the launch plan, the descriptor uploads, `hook`, the TLS 1.3 header kernel, the record kernel (batch.cpp's
 * launch_plan: the pipeline waits for every slice itself and notes no keyset use) and the inner-plaintext kernel, in that
 * order on s.stream.  in / aad / out / result / mask are device addresses: of the caller's mapped buffers, or of the slot's
 * staging.  `hook(plan)` queues what the transport itself uploads for the slice (copy: the records' bytes and the gaps), and
 * for QUIC open the header step, between the descriptor uploads and the kernels, where they always were queued.
 * An AES-GCM slice is planned like a batch (lanes: mapped_lanes or choose_lanes; chunks; the order, uploaded only when it is
 * not the identity); a ChaCha slice has no launch plan (the kernels take the records in descriptor order, as in run_batch: no
 * chunks, no order, no chunk queue), only chacha_plan's width and layout.
 * The ALIGNED kernels also need 16-byte aligned bases, which launch_plan tests.  The mapped transport's are the caller's
 * buffers; the copy transport's are hipMalloc'd staging, always aligned (its slice-local offsets keep the caller's alignment
 * modulo 16, slice_plan.cpp), so there the descriptors alone decide, as they always did. */
template <class Hook>
static int launch_slice(ptls_hip_pipeline_t *p, PipeSlot &s, ptls_hip_keyset_t *ks, size_t cnt, const ModeInfo &m, const uint8_t *in,
                        const uint8_t *aad, uint8_t *out, uint64_t *result, ptls_hip_keyset_t *hp_ks, bool have_supp, uint8_t *mask,
                        bool mapped, Hook hook)
{
    const unsigned ncu = (unsigned)p->eng->ncu;
    LaunchPlan lp{};
    lp.eng = p->eng;
    lp.n = cnt;
    lp.d_recs = s.d_recs;
    lp.ncus = ncu;
    const bool chacha = ks->algo == PTLS_HIP_ALGO_CHACHA20POLY1305;
    if (chacha) {
        const ChaChaPlan c = chacha_plan(p, s.h_recs, cnt, mapped);
        lp.chacha_lanes = c.lanes;
        lp.chacha_runs = c.runs; /* (all_aligned: below) */
    } else {
        lp.lanes = mapped ? mapped_lanes(s.h_recs, cnt, ncu) : choose_lanes(s.h_recs, cnt, ncu);
        build_chunks(s.h_recs, cnt, lp.lanes, ncu, p->ch, p->order, lp.all_aligned);
        lp.wg = plan_wg(p->ch, lp.lanes);
        lp.d_chunks = s.d_chunks;
        lp.nchunks = (uint32_t)p->ch.size();
        std::memcpy(s.h_chunks, p->ch.data(), p->ch.size() * sizeof(Chunk));
        if (!identity_order(p->order, cnt)) {
            lp.d_recs_ord = s.d_recs_ord;
            lp.d_order = s.d_order;
            std::memcpy(s.h_order, p->order.data(), cnt * sizeof(uint32_t));
            for (size_t t = 0; t < cnt; ++t)
                s.h_recs_ord[t] = s.h_recs[p->order[t]];
            HIP_TRY(hipMemcpyAsync(s.d_recs_ord, s.h_recs_ord, cnt * sizeof(ptls_hip_record_t), hipMemcpyHostToDevice, s.stream),
                    PTLS_HIP_ENODEV);
            HIP_TRY(hipMemcpyAsync(s.d_order, s.h_order, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, s.stream), PTLS_HIP_ENODEV);
        }
    }
    HIP_TRY(hipMemcpyAsync(s.d_recs, s.h_recs, cnt * sizeof(ptls_hip_record_t), hipMemcpyHostToDevice, s.stream), PTLS_HIP_ENODEV);
    if (lp.nchunks != 0)
        HIP_TRY(hipMemcpyAsync(s.d_chunks, s.h_chunks, lp.nchunks * sizeof(Chunk), hipMemcpyHostToDevice, s.stream), PTLS_HIP_ENODEV);
    if (have_supp)
        HIP_TRY(hipMemcpyAsync(s.d_supp, s.h_supp, cnt * sizeof(ptls_hip_supp_t), hipMemcpyHostToDevice, s.stream), PTLS_HIP_ENODEV);
    if (int rc = hook(lp))
        return rc;
    const unsigned egrid = record_grid(cnt, p->eng->ncu);
    if (m.aad_in_out && !m.quic) { /* TLS 1.3 seal: the headers, which the record kernel reads back as the AAD */
        const int eh = launch_tls13_headers(s.d_recs, (uint32_t)cnt, out, egrid, s.stream);
        if (eh != 0)
            return fail(PTLS_HIP_ELAUNCH, "pipeline: header kernel launch failed: %s", hipGetErrorString((hipError_t)eh));
    }
    /* A ChaCha slice's descriptors are scanned here, behind the uploads, so that the scan overlaps them: a slice of short
     * records is host-bound, and scanned before the uploads 4M x 256 B mapped lost 2.5 % (21.7 -> 21.1 GiB/s seal+open,
     * profiles/launch_plan_refactor_ab.log, first series) */
    if (chacha)
        lp.all_aligned = offsets_aligned(s.h_recs, cnt);
    if (int rc = launch_plan(lp, ks, in, m.aad_in_out ? out : m.aad_in_in ? in : aad, out, result, s.stream, m.open, hp_ks,
                             have_supp ? s.d_supp : nullptr, have_supp ? mask : nullptr))
        return rc;
    if (m.aad_in_in && !m.quic) { /* TLS 1.3 open: strip the inner plaintext's padding and content type */
        const int ei = launch_tls13_inner(s.d_recs, (uint32_t)cnt, out, result, egrid, s.stream);
        if (ei != 0)
            return fail(PTLS_HIP_ELAUNCH, "pipeline: inner-plaintext kernel launch failed: %s", hipGetErrorString((hipError_t)ei));
    }
    return 0;
}

/* The slice loop of every transport: slices rotate over the slots' streams, so the host plans and uploads slice k + 1
 * while the device runs k.  Per slice: plan(i, j) cuts records [i, j) on the host alone, refusals included, while the slot's
 * previous slice may still run; only then the slot is waited for; enqueue(s, i, j - i) fills the slot's staging and queues the
 * slice on s.stream.  At the end every slot is waited for: a kernel's stores to host memory are complete once its stream
 * event has been waited for.  After an error the caller drains the slots (drain_slots). */
template <class Plan, class Enqueue>
static int run_slices(ptls_hip_pipeline_t *p, size_t n, Plan plan, Enqueue enqueue)
{
    int k = 0;
    for (size_t i = 0, j = 0; i < n; i = j, ++k) {
        if (int rc = plan(i, j))
            return rc;
        PipeSlot &s = p->slot[k % NSLOT];
        if (int rc = slot_wait(s))
            return rc;
        if (int rc = enqueue(s, i, j - i))
            return rc;
        if (int rc = slot_submit(s))
            return rc;
    }
    for (auto &s : p->slot)
        if (int rc = slot_wait(s))
            return rc;
    return 0;
}

/* the mapped transports' greedy cut from record i: at most `cap` records and 4 x slice_bytes of payload.  4 x the staging
 * slice: no staging is involved, and the measured best (seal+open GiB/s of 1 GiB, 64 / 128 / 256 / 512 / 2048 MiB slices:
 * 16-KiB records 35.5 / 38.6 / 39.8 / 39.9 / 39.6, 1350-B records 32.9 / 33.3 / 33.4 / 30.7 / 21.9, configs[3] 34.7 / 36.3 /
 * 37.2 / 35.8 / 33.9) */
static size_t mapped_cut(const ptls_hip_pipeline_t *p, const ptls_hip_record_t *recs, size_t n, size_t i, size_t cap)
{
    const size_t mslice = 4 * p->slice_bytes;
    size_t cnt = 0, bytes = 0;
    while (i + cnt < n && cnt < cap && (cnt == 0 || bytes + recs[i + cnt].len <= mslice))
        bytes += recs[i + cnt++].len;
    return i + cnt;
}

/* PTLS_HIP_TRANSPORT_MAPPED: the batch kernel reads the records from, and writes them to, the caller's pinned host
 * buffers over PCIe itself (their device addresses); no staging copies, no copy engines.  Only the descriptors,
 * the launch plan and the header-protection descriptors go through the slots' pinned staging.  Slices of at
 * most 4 x slice_bytes of payload rotate over the slots' streams, so planning overlaps the kernels.  (tools/hostmem_probe.py,
 * the copy engines carry ~57 GB/s in both directions together, the kernel's own PCIe reads + writes
 * ~80 GB/s.) */
static int pipeline_run_mapped(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, const ptls_hip_record_t *recs, size_t n,
                               const uint8_t *d_in, const uint8_t *d_aad, uint8_t *d_out, uint64_t *h_result, uint64_t *d_res,
                               const ModeInfo &m, ptls_hip_keyset_t *hp_ks, const ptls_hip_supp_t *supp, uint8_t *d_mask)
{
    auto plan = [&](size_t i, size_t &j) { return j = mapped_cut(p, recs, n, i, p->max_recs - 1), 0; };
    auto enqueue = [&](PipeSlot &s, size_t i, size_t cnt) -> int {
        std::memcpy(s.h_recs, recs + i, cnt * sizeof(ptls_hip_record_t));
        if (supp != nullptr)
            std::memcpy(s.h_supp, supp + i, cnt * sizeof(ptls_hip_supp_t));
        /* results go straight to mapped memory, or through the slot when h_result is not mapped */
        uint64_t *res = d_res != nullptr ? d_res + i : s.d_result;
        if (int rc = launch_slice(p, s, ks, cnt, m, d_in, d_aad, d_out, res, hp_ks, supp != nullptr, d_mask, true,
                                  [](const LaunchPlan &) { return 0; }))
            return rc;
        if (m.open && d_res == nullptr)
            HIP_TRY(hipMemcpyAsync(h_result + i, s.d_result, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream),
                    PTLS_HIP_ENODEV);
        return 0;
    };
    if (int rc = run_slices(p, n, plan, enqueue))
        return rc;
    p->last_transport = PTLS_HIP_TRANSPORT_MAPPED;
    return 0;
}

/* the copy transport's staging for gaps and masks (slice_plan.cpp), allocated on the first slice that needs it */
static int slot_mask_buffer(ptls_hip_pipeline_t *p, PipeSlot &s)
{
    if (s.h_mask != nullptr)
        return 0;
    if (hipHostMalloc(&s.h_mask, slot_max_masks(p->slice_bytes) * 16, hipHostMallocDefault) != hipSuccess) {
        s.h_mask = nullptr;
        return fail(PTLS_HIP_ENOMEM, "pipeline: cannot allocate the copy transport's mask staging");
    }
    return 0;
}

static int slot_gap_buffers(ptls_hip_pipeline_t *p, PipeSlot &s)
{
    if (s.h_gap != nullptr)
        return 0;
    const size_t npieces = 2 * p->max_recs;
    if (hipHostMalloc(&s.h_gap, p->slice_bytes, hipHostMallocDefault) != hipSuccess ||
        hipMalloc(&s.d_gap, p->slice_bytes) != hipSuccess ||
        hipHostMalloc(&s.h_gapd, npieces * sizeof(GapPiece), hipHostMallocDefault) != hipSuccess ||
        hipMalloc(&s.d_gapd, npieces * sizeof(GapPiece)) != hipSuccess) {
        (void)hipHostFree(s.h_gap);
        (void)hipFree(s.d_gap);
        (void)hipHostFree(s.h_gapd);
        (void)hipFree(s.d_gapd);
        s.h_gap = s.d_gap = nullptr;
        s.h_gapd = s.d_gapd = nullptr;
        return fail(PTLS_HIP_ENOMEM, "pipeline: cannot allocate the copy transport's gap staging");
    }
    return 0;
}

/* a copy-transport slice's gaps (and what a QUIC slice stages with them, plan_quic_slice): the caller's bytes of h_out,
 * gathered into the slot's pinned gap staging, uploaded and placed in d_out by gap_scatter_kernel, on s.stream before the
 * slice's kernels */
static int stage_gaps(ptls_hip_pipeline_t *p, PipeSlot &s, const SlicePlan &pl, const uint8_t *hout)
{
    const size_t ngap = pl.gaps.size();
    if (ngap == 0)
        return 0;
    /* The gap staging is allocated here, behind the slot's first payload upload, where it always was, and not with
     * the mask staging before the first enqueue.  Measured: allocated before the slot's first enqueue, every later
     * slice's copies start only when the previous slice's copy back has ended, on any of the three streams (c2 copy
     * seal+open 28.2 -> 24.0 GiB/s, same kernels and copies in the traces; profiles/pipeline_refactor_ab.log).
     * Supposed cause: on a slot's first slice these milliseconds let its upload finish before the other slots make
     * their first copies, and the runtime binds a stream to a copy engine at its first copy.  If the allocation
     * fails, drain_slots waits for the uploads already queued. */
    if (int rc = slot_gap_buffers(p, s))
        return rc;
    /* the caller's bytes of the gaps as they are now: no slice in flight writes them (plan_copy_slice fills no gap
     * that another slice's record touches) */
    for (size_t t = 0; t < ngap; ++t) {
        s.h_gapd[t] = pl.gaps[t];
        std::memcpy(s.h_gap + pl.gaps[t].src, hout + pl.gap_src[t].lo, pl.gaps[t].len);
    }
    const GapPiece &last = pl.gaps.back();
    HIP_TRY(hipMemcpyAsync(s.d_gapd, s.h_gapd, ngap * sizeof(GapPiece), hipMemcpyHostToDevice, s.stream), PTLS_HIP_ENODEV);
    HIP_TRY(hipMemcpyAsync(s.d_gap, s.h_gap, (size_t)last.src + last.len, hipMemcpyHostToDevice, s.stream), PTLS_HIP_ENODEV);
    const int eg = launch_gap_scatter(s.d_gapd, (uint32_t)ngap, s.d_gap, s.d_out, s.stream);
    return eg == 0 ? 0 : fail(PTLS_HIP_ELAUNCH, "pipeline: gap-fill kernel launch failed: %s", hipGetErrorString((hipError_t)eg));
}

/* PTLS_HIP_TRANSPORT_COPY: slices staged through the slots' device buffers by the copy engines.  Per slice: its plan
 * first (plan_copy_slice, refusals included, while the slot's previous slice still runs), then the slot and its mask
 * staging, and only then the slice's first enqueue; after that nothing but a HIP call (an enqueue, or the first
 * allocation of a slot's gap staging) can fail, and drain_slots waits for every stream. */
static int pipeline_run_copy(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, const ptls_hip_record_t *recs, size_t n,
                             const void *h_in, const void *h_aad, void *h_out, uint64_t *h_result, const ModeInfo &m,
                             ptls_hip_keyset_t *hp_ks, const ptls_hip_supp_t *supp, void *h_mask)
{
    p->last_transport = PTLS_HIP_TRANSPORT_COPY;
    const uint8_t *hin = static_cast<const uint8_t *>(h_in), *haad = static_cast<const uint8_t *>(h_aad);
    uint8_t *hout = static_cast<uint8_t *>(h_out);
    CopyOrder ord;
    plan_copy_order(recs, n, m, ord);
    SlicePlan pl;
    auto plan = [&](size_t i, size_t &j) {
        const int rc = plan_copy_slice(recs, supp, n, i, m, p->slice_bytes, p->max_recs, hp_ks != nullptr ? hp_ks->nslots : 0, ord, pl);
        j = pl.j;
        return rc;
    };
    auto enqueue = [&](PipeSlot &s, size_t i, size_t cnt) -> int {
        if (!pl.mask_dst.empty())
            if (int rc = slot_mask_buffer(p, s))
                return rc;
        /* the slot's pinned staging: descriptors and mask places */
        std::memcpy(s.h_recs, pl.recs.data(), cnt * sizeof(ptls_hip_record_t));
        if (supp != nullptr)
            std::memcpy(s.h_supp, pl.supp.data(), cnt * sizeof(ptls_hip_supp_t));
        s.mask_host = static_cast<uint8_t *>(h_mask);
        s.mask_dst.swap(pl.mask_dst);
        auto payload = [&](const LaunchPlan &) -> int {
            HIP_TRY(hipMemcpyAsync(s.d_in + (pl.in.lo - pl.in_base), hin + pl.in.lo, pl.in.hi - pl.in.lo, hipMemcpyHostToDevice, s.stream),
                    PTLS_HIP_ENODEV);
            if (pl.aad.hi > pl.aad.lo)
                HIP_TRY(hipMemcpyAsync(s.d_aad + (pl.aad.lo - pl.aad_base), haad + pl.aad.lo, pl.aad.hi - pl.aad.lo,
                                       hipMemcpyHostToDevice, s.stream),
                        PTLS_HIP_ENODEV);
            return stage_gaps(p, s, pl, hout);
        };
        if (int rc = launch_slice(p, s, ks, cnt, m, s.d_in, s.d_aad, s.d_out, s.d_result, hp_ks, supp != nullptr, s.d_mask, false, payload))
            return rc;
        for (const Span &pc : pl.pieces)
            HIP_TRY(hipMemcpyAsync(hout + pc.lo, s.d_out + (pc.lo - pl.out_base), pc.hi - pc.lo, hipMemcpyDeviceToHost, s.stream),
                    PTLS_HIP_ENODEV);
        if (!s.mask_dst.empty()) /* the slice's masks, packed: one copy; slot_wait places them */
            HIP_TRY(hipMemcpyAsync(s.h_mask, s.d_mask, 16 * s.mask_dst.size(), hipMemcpyDeviceToHost, s.stream), PTLS_HIP_ENODEV);
        if (m.open) /* results come back in slice order; the caller's array is indexed like recs */
            HIP_TRY(hipMemcpyAsync(h_result + i, s.d_result, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream),
                    PTLS_HIP_ENODEV);
        return 0;
    };
    return run_slices(p, n, plan, enqueue);
}

static int pipeline_run(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, const ptls_hip_record_t *recs, size_t n, const void *h_in,
                        const void *h_aad, void *h_out, uint64_t *h_result, PipeMode mode, ptls_hip_keyset_t *hp_ks = nullptr,
                        const ptls_hip_supp_t *supp = nullptr, void *h_mask = nullptr)
{
    /* a pipeline serves the keysets of the algorithm it was made for (ptls_hip_pipeline_new: AES-GCM): its slots hold what
     * that algorithm's launches need */
    const int algo = p != nullptr ? p->algo : PTLS_HIP_ALGO_AESGCM;
    if ((ks != nullptr && ks->algo != algo) || (hp_ks != nullptr && hp_ks->algo != algo))
        return fail(PTLS_HIP_EINVAL, "pipeline: this pipeline serves %s keysets (ptls_hip_pipeline_new_algo)",
                    algo == PTLS_HIP_ALGO_CHACHA20POLY1305 ? "ChaCha20-Poly1305" : "AES-GCM");
    if (supp != nullptr && (mode != PIPE_SEAL || hp_ks == nullptr || ks == nullptr || hp_ks->eng != ks->eng ||
                            hp_ks->key_size != ks->key_size || h_mask == nullptr))
        return fail(PTLS_HIP_EINVAL, "pipeline_seal_supp: the header-protection keyset must be on the same engine with the "
                                     "AEAD's key size, and h_mask must be given");
    const ModeInfo m(mode);
    if (p == nullptr || ks == nullptr || ks->eng != p->eng || (n != 0 && (recs == nullptr || h_in == nullptr || h_out == nullptr)) ||
        (m.open && h_result == nullptr))
        return fail(PTLS_HIP_EINVAL, "pipeline seal/open: bad arguments");
    for (size_t i = 0; i < n; ++i)
        if (recs[i].key >= ks->nslots)
            return fail(PTLS_HIP_EINVAL, "pipeline: record %zu names key slot %u, the keyset has %zu", i, recs[i].key, ks->nslots);
    DeviceGuard g(p->eng->device);
    /* every transport checks the buffers: the copy engines refuse a buffer registered only in part as well (hipMemcpyAsync:
     * invalid argument, tests/test_gpu_node.py::test_partly_registered_input_is_refused), so such a call fails here with
     * a message that names the cause; unregistered (pageable) buffers go to the copy transport */
    if (n != 0) {
        /* the bytes the kernels would touch in each buffer: [base, base + need) */
        uint64_t need_in = 0, need_out = 0, need_aad = 0, need_mask = 0;
        for (size_t i = 0; i < n; ++i) {
            const ptls_hip_record_t &r = recs[i];
            need_in = std::max<uint64_t>(need_in, r.in_off + r.len + m.tag_in);
            need_out = std::max<uint64_t>(need_out, r.out_off + r.len + m.tag_out);
            if (r.aad_len != 0) {
                uint64_t &na = m.aad_in_out ? need_out : m.aad_in_in ? need_in : need_aad;
                na = std::max<uint64_t>(na, r.aad_off + r.aad_len);
            }
            if (supp != nullptr && (supp[i].flags & PTLS_HIP_SUPP_ENABLE))
                need_mask = std::max<uint64_t>(need_mask, supp[i].mask_off + 16);
        }
        bool partial = false;
        const uint8_t *d_in = static_cast<const uint8_t *>(mapped_span(h_in, need_in, &partial));
        uint8_t *d_out = static_cast<uint8_t *>(mapped_span(h_out, need_out, &partial));
        const uint8_t *d_aad = static_cast<const uint8_t *>(mapped_span(h_aad, need_aad, &partial));
        uint8_t *d_mask = static_cast<uint8_t *>(mapped_span(h_mask, need_mask, &partial));
        uint64_t *d_res = m.open ? static_cast<uint64_t *>(mapped_span(h_result, (uint64_t)n * 8, &partial)) : nullptr;
        if (partial)
            return refuse_partial();
        const bool ok = d_in != nullptr && d_out != nullptr && (h_aad == nullptr || d_aad != nullptr) && (h_mask == nullptr || d_mask != nullptr);
        if (ok && p->transport != PTLS_HIP_TRANSPORT_COPY) {
            const int rc = pipeline_run_mapped(p, ks, recs, n, d_in, d_aad, d_out, h_result, d_res, m, hp_ks, supp, d_mask);
            if (rc != 0)
                drain_slots(p);
            return rc;
        }
        if (p->transport == PTLS_HIP_TRANSPORT_MAPPED)
            return fail(PTLS_HIP_EINVAL, "pipeline: transport MAPPED needs host buffers (in, out, aad, mask) pinned or registered "
                                         "over every byte the records touch");
    }
    const int rc = pipeline_run_copy(p, ks, recs, n, h_in, h_aad, h_out, h_result, m, hp_ks, supp, h_mask);
    if (rc != 0)
        drain_slots(p);
    return rc;
}

extern "C" int ptls_hip_pipeline_seal(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, const ptls_hip_record_t *recs, size_t n,
                                      const void *h_in, const void *h_aad, void *h_out)
{
    return pipeline_run(p, ks, recs, n, h_in, h_aad, h_out, nullptr, PIPE_SEAL);
}

extern "C" int ptls_hip_pipeline_seal_supp(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                                           const ptls_hip_record_t *recs, const ptls_hip_supp_t *supp, size_t n, const void *h_in,
                                           const void *h_aad, void *h_out, void *h_mask)
{
    if (n != 0 && supp == nullptr)
        return fail(PTLS_HIP_EINVAL, "pipeline_seal_supp: supp descriptors missing");
    return pipeline_run(p, ks, recs, n, h_in, h_aad, h_out, nullptr, PIPE_SEAL, hp_ks, supp, h_mask);
}

extern "C" int ptls_hip_pipeline_tls13_seal(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, const ptls_hip_record_t *recs, size_t n,
                                            const void *h_in, void *h_wire)
{
    return pipeline_run(p, ks, recs, n, h_in, nullptr, h_wire, nullptr, PIPE_TLS13_SEAL);
}

extern "C" int ptls_hip_pipeline_tls13_open(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, const ptls_hip_record_t *recs, size_t n,
                                            const void *h_wire, void *h_out, uint64_t *h_result)
{
    return pipeline_run(p, ks, recs, n, h_wire, nullptr, h_out, h_result, PIPE_TLS13_OPEN);
}

extern "C" int ptls_hip_pipeline_open(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, const ptls_hip_record_t *recs, size_t n,
                                      const void *h_in, const void *h_aad, void *h_out, uint64_t *h_result)
{
    return pipeline_run(p, ks, recs, n, h_in, h_aad, h_out, h_result, PIPE_OPEN);
}

/* ---------------------------------------------------------------------------------------------- */
/* QUIC packets from and to host memory (include/ptls_hip.h 2g)                    */
/* ---------------------------------------------------------------------------------------------- */

/* the slot's staging for QUIC slices, allocated before the first enqueue of the slot's first such slice (as the mask
 * staging is): at most slot_max_masks packets per slice on either transport */
static int slot_quic_buffers(ptls_hip_pipeline_t *p, PipeSlot &s, bool open)
{
    const size_t cap = slot_max_masks(p->slice_bytes);
    if (s.h_pkts == nullptr &&
        (hipHostMalloc(&s.h_pkts, cap * sizeof(ptls_hip_quic_packet_t), hipHostMallocDefault) != hipSuccess ||
         hipMalloc(&s.d_pkts, cap * sizeof(ptls_hip_quic_packet_t)) != hipSuccess)) {
        (void)hipHostFree(s.h_pkts);
        (void)hipFree(s.d_pkts);
        s.h_pkts = s.d_pkts = nullptr;
        return fail(PTLS_HIP_ENOMEM, "pipeline: cannot allocate the packet descriptor staging");
    }
    if (open && s.d_pn == nullptr &&
        (hipMalloc(&s.d_pn, cap * sizeof(uint64_t)) != hipSuccess || hipMalloc(&s.d_hdr, cap * 8) != hipSuccess ||
         hipHostMalloc(&s.h_hdr, cap * 8, hipHostMallocDefault) != hipSuccess)) {
        (void)hipFree(s.d_pn);
        (void)hipFree(s.d_hdr);
        (void)hipHostFree(s.h_hdr);
        s.d_pn = nullptr;
        s.d_hdr = s.h_hdr = nullptr;
        return fail(PTLS_HIP_ENOMEM, "pipeline: cannot allocate the packet-number and header staging");
    }
    return 0;
}

/* One slice of cnt packets on slot s, the same for both transports, once s.h_pkts, s.h_recs (and for seal s.h_supp: sample
 * at pn_offset + 4, mask t at 16 t of s.d_mask) hold its slice-local descriptors.  On s.stream, through launch_slice:
 *   seal: descriptors, `upload`, the record kernel with the header-protection masks (AAD = the header in pkt, where the
 *         output goes), quic_protect_kernel;
 *   open: descriptors, `upload`, quic_unprotect_kernel (it rewrites the slice's d_recs, and d_recs_ord through d_order when
 *         the launch plan has an order: launch_slice uploaded the provisional ones before its hook), on the copy transport
 *         quic_pack_headers_kernel (`packed`), then the record open kernel (input and AAD in pkt).
 * `upload` queues what the transport itself uploads.  in / pkt / out / result / pn_out are device addresses. */
template <class Upload>
static int launch_quic_slice(ptls_hip_pipeline_t *p, PipeSlot &s, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, size_t cnt,
                             const ModeInfo &m, const uint8_t *in, uint8_t *pkt, uint8_t *out, uint64_t *result, uint64_t *pn_out,
                             uint8_t *packed, bool mapped, Upload upload)
{
    HIP_TRY(hipMemcpyAsync(s.d_pkts, s.h_pkts, cnt * sizeof(ptls_hip_quic_packet_t), hipMemcpyHostToDevice, s.stream), PTLS_HIP_ENODEV);
    auto between = [&](const LaunchPlan &lp) -> int {
        if (int rc = upload())
            return rc;
        if (!m.open)
            return 0;
        int e = quic_unprotect(p->eng, hp_ks, s.d_pkts, cnt, lp.d_recs, lp.d_recs_ord, lp.d_order, pkt, pn_out, s.stream);
        if (e == 0 && packed != nullptr)
            e = launch_quic_pack_headers(s.d_pkts, (uint32_t)cnt, pkt, packed, s.stream);
        return e == 0 ? 0 : fail(PTLS_HIP_ELAUNCH, "pipeline_quic_open: header kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    };
    if (m.open)
        return launch_slice(p, s, ks, cnt, m, pkt, nullptr, out, result, nullptr, false, nullptr, mapped, between);
    if (int rc = launch_slice(p, s, ks, cnt, m, in, nullptr, pkt, nullptr, hp_ks, true, s.d_mask, mapped, between))
        return rc;
    const int e = quic_protect(s.d_pkts, cnt, pkt, s.d_mask, s.stream);
    return e == 0 ? 0 : fail(PTLS_HIP_ELAUNCH, "pipeline_quic_seal: header kernel launch failed: %s", hipGetErrorString((hipError_t)e));
}

/* the slice's descriptors into the slot's pinned staging: records and packets [i, i + cnt) in the offsets the kernels will
 * use.  open: the provisional records are marked not 16-byte aligned (the real in_off is known only to
 * quic_unprotect_kernel, and launch_slice takes `all_aligned` from these host descriptors);
 * seal: mask t of the slice at 16 t of the slot's d_mask */
static void fill_quic_slot(PipeSlot &s, const ptls_hip_record_t *recs, const ptls_hip_supp_t *supp,
                           const ptls_hip_quic_packet_t *pkts, size_t cnt, const ModeInfo &m)
{
    std::memcpy(s.h_recs, recs, cnt * sizeof(ptls_hip_record_t));
    std::memcpy(s.h_pkts, pkts, cnt * sizeof(ptls_hip_quic_packet_t));
    for (size_t t = 0; t < cnt; ++t) {
        if (m.open) {
            s.h_recs[t].in_off |= 1u;
        } else {
            s.h_supp[t] = supp[t];
            s.h_supp[t].mask_off = 16 * (uint64_t)t;
        }
    }
}

/* MAPPED: the kernels run on the buffers' device addresses with the caller's offsets, the header kernels too (they read and
 * rewrite the header bytes in host memory over PCIe); the masks stay in the slot's d_mask.  Slices of at most 4 x
 * slice_bytes of payload and slot_max_masks packets.  Results and packet numbers go straight to mapped arrays, or through
 * the slot when the caller's are not mapped. */
static int quic_run_mapped(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, const ptls_hip_quic_packet_t *pkts,
                           const ptls_hip_record_t *recs, const ptls_hip_supp_t *supp, size_t n, const ModeInfo &m,
                           const uint8_t *d_in, uint8_t *d_pkt, uint8_t *d_out, uint64_t *h_result, uint64_t *d_res,
                           uint64_t *h_pn, uint64_t *d_pn)
{
    auto plan = [&](size_t i, size_t &j) { return j = mapped_cut(p, recs, n, i, slot_max_masks(p->slice_bytes)), 0; };
    auto enqueue = [&](PipeSlot &s, size_t i, size_t cnt) -> int {
        if (int rc = slot_quic_buffers(p, s, m.open))
            return rc;
        fill_quic_slot(s, recs + i, m.open ? nullptr : supp + i, pkts + i, cnt, m);
        uint64_t *res = d_res != nullptr ? d_res + i : s.d_result, *pn = d_pn != nullptr ? d_pn + i : s.d_pn;
        if (int rc = launch_quic_slice(p, s, ks, hp_ks, cnt, m, d_in, d_pkt, d_out, res, pn, nullptr, true, [] { return 0; }))
            return rc;
        if (m.open && d_res == nullptr)
            HIP_TRY(hipMemcpyAsync(h_result + i, s.d_result, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream), PTLS_HIP_ENODEV);
        if (m.open && d_pn == nullptr)
            HIP_TRY(hipMemcpyAsync(h_pn + i, s.d_pn, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream), PTLS_HIP_ENODEV);
        return 0;
    };
    if (int rc = run_slices(p, n, plan, enqueue))
        return rc;
    p->last_transport = PTLS_HIP_TRANSPORT_MAPPED;
    return 0;
}

/* COPY: per slice its plan (plan_quic_slice), the slot and its staging, then on the slot's stream the input span (seal: the
 * payloads; open: the packets), the gaps with the headers (seal) or the plaintext tails (open), the kernels, and the
 * copies back: seal the packets' merged runs; open the plaintext areas' merged runs at their pn_len = 1 length, the packed
 * header entries (slot_wait places them in h_pkt), the results and the packet numbers. */
static int quic_run_copy(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, const ptls_hip_quic_packet_t *pkts,
                         const ptls_hip_record_t *recs, const ptls_hip_supp_t *supp, size_t n, const ModeInfo &m, const uint8_t *h_in,
                         uint8_t *h_pkt, uint8_t *h_out, uint64_t *h_result, uint64_t *h_pn)
{
    p->last_transport = PTLS_HIP_TRANSPORT_COPY;
    const uint8_t *hin = m.open ? h_pkt : h_in; /* what the slice uploads a span of */
    uint8_t *hout = m.open ? h_out : h_pkt;     /* where its output goes, and where its gaps come from */
    CopyOrder ord;
    plan_copy_order(recs, n, m, ord);
    QuicSlicePlan pl;
    auto plan = [&](size_t i, size_t &j) {
        const int rc = plan_quic_slice(pkts, recs, supp, n, i, m, p->slice_bytes, p->max_recs, ord, pl);
        j = pl.s.j;
        return rc;
    };
    auto enqueue = [&](PipeSlot &s, size_t i, size_t cnt) -> int {
        if (int rc = slot_quic_buffers(p, s, m.open))
            return rc;
        fill_quic_slot(s, pl.s.recs.data(), pl.s.supp.data(), pl.pkts.data(), cnt, m);
        s.hdr_host = h_pkt;
        s.hdr_dst.swap(pl.hdr_dst);
        auto upload = [&]() -> int {
            if (pl.s.in.hi > pl.s.in.lo)
                HIP_TRY(hipMemcpyAsync(s.d_in + (pl.s.in.lo - pl.s.in_base), hin + pl.s.in.lo, pl.s.in.hi - pl.s.in.lo,
                                       hipMemcpyHostToDevice, s.stream),
                        PTLS_HIP_ENODEV);
            return stage_gaps(p, s, pl.s, hout);
        };
        if (int rc = launch_quic_slice(p, s, ks, hp_ks, cnt, m, s.d_in, m.open ? s.d_in : s.d_out, s.d_out, s.d_result, s.d_pn,
                                       m.open ? s.d_hdr : nullptr, false, upload))
            return rc;
        for (const Span &pc : pl.s.pieces)
            HIP_TRY(hipMemcpyAsync(hout + pc.lo, s.d_out + (pc.lo - pl.s.out_base), pc.hi - pc.lo, hipMemcpyDeviceToHost, s.stream),
                    PTLS_HIP_ENODEV);
        if (m.open) {
            HIP_TRY(hipMemcpyAsync(s.h_hdr, s.d_hdr, 8 * cnt, hipMemcpyDeviceToHost, s.stream), PTLS_HIP_ENODEV);
            HIP_TRY(hipMemcpyAsync(h_result + i, s.d_result, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream), PTLS_HIP_ENODEV);
            HIP_TRY(hipMemcpyAsync(h_pn + i, s.d_pn, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream), PTLS_HIP_ENODEV);
        }
        return 0;
    };
    return run_slices(p, n, plan, enqueue);
}

/* both calls: every refusal comes before anything is launched, copied or written */
static int pipeline_quic_run(const char *who, ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                             const ptls_hip_quic_packet_t *pkts, size_t n, PipeMode mode, const void *h_in, void *h_pkt, void *h_out,
                             uint64_t *h_result, uint64_t *h_pn)
{
    const ModeInfo m(mode);
    if (p == nullptr || ks == nullptr || hp_ks == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null pipeline or keyset", who);
    if (n != 0 && (pkts == nullptr || h_pkt == nullptr ||
                   (m.open ? h_out == nullptr || h_result == nullptr || h_pn == nullptr : h_in == nullptr)))
        return fail(PTLS_HIP_EINVAL, "%s: null buffer", who);
    if (ks->eng != p->eng || hp_ks->eng != p->eng)
        return fail(PTLS_HIP_EINVAL, "%s: pipeline and keysets must belong to the same engine", who);
    if (hp_ks->algo != ks->algo || hp_ks->key_size != ks->key_size)
        return fail(PTLS_HIP_EINVAL, "%s: the header-protection keyset must be of the AEAD keyset's algorithm and key size", who);
    if (ks->algo != p->algo)
        return fail(PTLS_HIP_EINVAL, "pipeline: this pipeline serves %s keysets (ptls_hip_pipeline_new_algo)",
                    p->algo == PTLS_HIP_ALGO_CHACHA20POLY1305 ? "ChaCha20-Poly1305" : "AES-GCM");
    if (n == 0)
        return 0;
    for (size_t i = 0; i < n; ++i) {
        if (const char *why = quic_packet_fault(pkts[i], m.open))
            return fail(PTLS_HIP_EINVAL, "%s: packet %zu: %s", who, i, why);
        if (pkts[i].key >= ks->nslots)
            return fail(PTLS_HIP_EINVAL, "%s: packet %zu names key slot %u, the keyset has %zu", who, i, pkts[i].key, ks->nslots);
        if (pkts[i].hp_key >= hp_ks->nslots)
            return fail(PTLS_HIP_EINVAL, "%s: packet %zu names header-protection key slot %u, the keyset has %zu", who, i,
                        pkts[i].hp_key, hp_ks->nslots);
    }
    std::vector<ptls_hip_record_t> recs;
    std::vector<ptls_hip_supp_t> supp;
    quic_records(pkts, n, m.open, recs, supp);
    /* the bytes the kernels would touch in each buffer: [base + lo, base + need) */
    uint64_t need_pkt = 0, need_data = 0, lo_pkt = UINT64_MAX, lo_data = UINT64_MAX;
    for (size_t i = 0; i < n; ++i) {
        need_pkt = std::max<uint64_t>(need_pkt, pkts[i].pkt_off + pkts[i].pkt_len);
        lo_pkt = std::min<uint64_t>(lo_pkt, pkts[i].pkt_off);
        need_data = std::max<uint64_t>(need_data, pkts[i].data_off + recs[i].len);
        lo_data = std::min<uint64_t>(lo_data, pkts[i].data_off);
    }
    if (m.open) { /* host addresses, so the ranges compare exactly */
        const uintptr_t pk = reinterpret_cast<uintptr_t>(h_pkt), ou = reinterpret_cast<uintptr_t>(h_out);
        if (ou + lo_data < pk + need_pkt && pk + lo_pkt < ou + need_data)
            return fail(PTLS_HIP_EINVAL, "%s: h_out overlaps the packets in h_pkt", who);
    }
    DeviceGuard g(p->eng->device);
    void *h_data = m.open ? h_out : const_cast<void *>(h_in);
    bool partial = false;
    uint8_t *d_pkt = static_cast<uint8_t *>(mapped_span(h_pkt, need_pkt, &partial));
    uint8_t *d_data = static_cast<uint8_t *>(mapped_span(h_data, need_data, &partial));
    uint64_t *d_res = m.open ? static_cast<uint64_t *>(mapped_span(h_result, (uint64_t)n * 8, &partial)) : nullptr;
    uint64_t *d_pn = m.open ? static_cast<uint64_t *>(mapped_span(h_pn, (uint64_t)n * 8, &partial)) : nullptr;
    if (partial)
        return refuse_partial();
    int rc;
    if (d_pkt != nullptr && d_data != nullptr && p->transport != PTLS_HIP_TRANSPORT_COPY) {
        rc = quic_run_mapped(p, ks, hp_ks, pkts, recs.data(), supp.data(), n, m, m.open ? nullptr : d_data, d_pkt,
                             m.open ? d_data : nullptr, h_result, d_res, h_pn, d_pn);
    } else {
        if (p->transport == PTLS_HIP_TRANSPORT_MAPPED)
            return fail(PTLS_HIP_EINVAL, "%s: transport MAPPED needs the host buffers (packets and payloads) pinned or registered "
                                         "over every byte the packets touch", who);
        for (size_t i = 0; i < n; ++i)
            if (pkts[i].pkt_len > p->slice_bytes)
                return fail(PTLS_HIP_EINVAL, "%s: packet %zu does not fit a %zu-byte slice", who, i, p->slice_bytes);
        rc = quic_run_copy(p, ks, hp_ks, pkts, recs.data(), supp.data(), n, m, static_cast<const uint8_t *>(h_in),
                           static_cast<uint8_t *>(h_pkt), static_cast<uint8_t *>(h_out), h_result, h_pn);
    }
    if (rc != 0)
        drain_slots(p);
    return rc;
}

extern "C" int ptls_hip_pipeline_quic_seal(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                                           const ptls_hip_quic_packet_t *pkts, size_t n, const void *h_in, void *h_pkt)
{
    return pipeline_quic_run("pipeline_quic_seal", p, ks, hp_ks, pkts, n, PIPE_QUIC_SEAL, h_in, h_pkt, nullptr, nullptr, nullptr);
}

extern "C" int ptls_hip_pipeline_quic_open(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                                           const ptls_hip_quic_packet_t *pkts, size_t n, void *h_pkt, void *h_out,
                                           uint64_t *h_result, uint64_t *h_pn_out)
{
    return pipeline_quic_run("pipeline_quic_open", p, ks, hp_ks, pkts, n, PIPE_QUIC_OPEN, nullptr, h_pkt, h_out, h_result, h_pn_out);
}
