/*
 * quic_tx.cpp -- the send object (include/ptls_hip.h 2l): requests in device memory become protected
 * short-header packets with one call.  The packet numbers, their encoded lengths, the header bytes and the key generation
 * come from a per-connection state table on the device (the rule: quic_tx.h, shared with quic_tx_kernel.hip); the compacted
 * descriptors then go through what every seal path here uses: the scan levels and the plan sort of quic_scratch.cpp (the
 * wave-per-record AES kernel's plan), batch.cpp's run_plan with header-protection masks, and
 * quic.cpp's quic_protect.  The host reads three sums per call and nothing per packet.
 */
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "host.h"

#define GF128_FN static inline
#include "quic_tx.h"

static_assert(sizeof(ptls_hip_quic_txconn_t) == 48 && __builtin_offsetof(ptls_hip_quic_txconn_t, gen) == 16 &&
                  __builtin_offsetof(ptls_hip_quic_txconn_t, dcid_len) == 20 && __builtin_offsetof(ptls_hip_quic_txconn_t, flags) == 21 &&
                  __builtin_offsetof(ptls_hip_quic_txconn_t, dcid) == 24,
              "ptls_hip_quic_txconn_t: 48 bytes, the connection ID at 24");
static_assert(sizeof(ptls_hip_quic_txreq_t) == 24 && __builtin_offsetof(ptls_hip_quic_txreq_t, pkt_off) == 8 &&
                  __builtin_offsetof(ptls_hip_quic_txreq_t, conn) == 16 && __builtin_offsetof(ptls_hip_quic_txreq_t, len) == 20,
              "ptls_hip_quic_txreq_t: 24 bytes");
static_assert(sizeof(ptls_hip_quic_tx_report_t) == 24, "ptls_hip_quic_tx_report_t: 24 bytes");

namespace {

thread_local bool g_timing = false;
thread_local float g_front_ms = 0, g_sort_ms = 0;

} // namespace

struct st_ptls_hip_quic_tx_t {
    ptls_hip_engine_t *eng;
    size_t cap;
    /* every d_ array below comes from here (tx_free: sc.release()); the timing events: the passes in front of the record
     * kernel 0-1, the sort 2-3 */
    DeviceScratch sc;
    size_t m = 0; /* sent packets of the last call: d_packed holds their descriptors */
    /* per request (cap): the two scan-level sets, the run starts (cap + 1) */
    uint32_t *d_run_levels = nullptr, *d_sent_levels = nullptr, *d_run_start = nullptr;
    /* per sent packet (cap) */
    ptls_hip_quic_packet_t *d_packed = nullptr;
    ptls_hip_record_t *d_recs = nullptr, *d_recs_ord = nullptr;
    ptls_hip_supp_t *d_supp = nullptr;
    uint8_t *d_mask = nullptr;
    uint32_t *d_keys = nullptr;
    PlanSort plan;
    uint64_t *d_stats = nullptr;
    Chunk *d_chunk = nullptr;
    /* per connection (first_cap): the position of its first run's head, QTX_NO_POS between calls */
    uint32_t *d_first = nullptr;
    size_t first_cap = 0;

    st_ptls_hip_quic_tx_t(ptls_hip_engine_t *e, size_t requests) : eng(e), cap(requests), sc(e, "quic_tx", 4) {}
};

extern "C" ptls_hip_quic_tx_t *ptls_hip_quic_tx_new(ptls_hip_engine_t *eng, size_t cap)
{
    if (eng == nullptr || cap < 1 || cap > 0xffffffffu) {
        fail(PTLS_HIP_EINVAL, "quic_tx_new: null engine, or cap %zu outside 1 .. 2^32 - 1", cap);
        return nullptr;
    }
    return new st_ptls_hip_quic_tx_t(eng, cap); /* device memory comes with the first use of each array */
}

extern "C" void ptls_hip_quic_tx_free(ptls_hip_quic_tx_t *tx)
{
    if (tx == nullptr)
        return;
    tx->sc.release();
    delete tx;
}

extern "C" const ptls_hip_quic_packet_t *ptls_hip_quic_tx_packets(ptls_hip_quic_tx_t *tx)
{
    return tx != nullptr && tx->m != 0 ? tx->d_packed : nullptr;
}

extern "C" size_t ptls_hip_quic_tx_count(ptls_hip_quic_tx_t *tx)
{
    return tx != nullptr ? tx->m : 0;
}

extern "C" void ptls_hip_quic_tx_timing(int enable, float *front_ms, float *sort_ms)
{
    g_timing = enable != 0;
    if (front_ms != nullptr)
        *front_ms = g_front_ms;
    if (sort_ms != nullptr)
        *sort_ms = g_sort_ms;
}

extern "C" int ptls_hip_quic_tx_seal(ptls_hip_quic_tx_t *tx, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                                     const ptls_hip_quic_tx_params_t *pr, const ptls_hip_quic_txreq_t *d_reqs, size_t n, const void *d_in,
                                     size_t in_len, void *d_pkt, size_t buf_len, ptls_hip_quic_tx_report_t *report, void *stream)
{
    const char *who = "quic_tx_seal";
    if (tx == nullptr || ks == nullptr || hp_ks == nullptr || pr == nullptr || report == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null send object, keyset, parameters or report", who);
    if (pr->d_conns == nullptr || pr->d_status == nullptr || pr->d_pn_out == nullptr || pr->d_pkt_len == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null state, status, packet-number or packet-length array", who);
    if (n > tx->cap)
        return fail(PTLS_HIP_EINVAL, "%s: %zu requests, the send object was made for %zu", who, n, tx->cap);
    if (pr->count == 0 || pr->count > 0xffffffffu)
        return fail(PTLS_HIP_EINVAL, "%s: a state count of %zu is outside 1 .. 2^32 - 1", who, pr->count);
    if (pr->stride == 0)
        return fail(PTLS_HIP_EINVAL, "%s: a bank stride of 0", who);
    if (pr->pn_len > 4)
        return fail(PTLS_HIP_EINVAL, "%s: pn_len %u is above 4", who, pr->pn_len);
    if (pr->reserved != 0)
        return fail(PTLS_HIP_EINVAL, "%s: params.reserved is not 0", who);
    if (int rc = quic_keysets_check(who, "send object", tx->eng, ks, hp_ks, pr->stride))
        return rc;
    if (n != 0 && (d_reqs == nullptr || d_in == nullptr || d_pkt == nullptr))
        return fail(PTLS_HIP_EINVAL, "%s: null request array or buffer", who);
    if (n != 0)
        if (int rc = quic_overlap_check(who, "packet buffer", d_pkt, buf_len, "payload buffer", d_in, in_len))
            return rc;
    report->n_sent = 0;
    report->bytes = 0;
    report->lanes = 0;
    report->reserved = 0;
    tx->m = 0;
    if (n == 0)
        return 0;

    ptls_hip_engine_t *eng = tx->eng;
    DeviceGuard g(eng->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t cap = tx->cap;
    const bool chacha = ks->algo == PTLS_HIP_ALGO_CHACHA20POLY1305;
    QuicTxLimits lim{};
    lim.in_len = in_len;
    lim.buf_len = buf_len;
    lim.nconn = (uint32_t)std::min(std::min(pr->count, pr->stride), std::min(hp_ks->nslots, (size_t)0xffffffffu));
    lim.stride = (uint32_t)pr->stride; /* 3 * stride <= nslots < 2^32 */
    lim.min_pn_len = pr->pn_len;
    lim.has_rx_phase = pr->d_rx_phase != nullptr ? 1u : 0u;

    const size_t level_words = scan_levels(nullptr, cap).words;
    int e = tx->sc.ensure_all({{&tx->d_run_levels, level_words * sizeof(uint32_t)}, {&tx->d_sent_levels, level_words * sizeof(uint32_t)},
                               {&tx->d_run_start, (cap + 1) * sizeof(uint32_t)}, {&tx->d_packed, cap * sizeof(ptls_hip_quic_packet_t)},
                               {&tx->d_recs, cap * sizeof(ptls_hip_record_t)}, {&tx->d_supp, cap * sizeof(ptls_hip_supp_t)},
                               {&tx->d_mask, cap * 16}, {&tx->d_keys, cap * sizeof(uint32_t)}, {&tx->d_stats, QTX_NSTATS * sizeof(uint64_t)}});
    if (e == 0 && !chacha) {
        e = tx->sc.ensure(&tx->d_recs_ord, cap * sizeof(ptls_hip_record_t));
        if (e == 0)
            e = tx->plan.ensure(tx->sc, cap, s);
        if (e == 0)
            e = tx->sc.ensure(&tx->d_chunk, sizeof(Chunk));
    }
    if (e != 0)
        return e;
    if (int e2 = tx->sc.grow(&tx->first_cap, lim.nconn, s, {{&tx->d_first, (size_t)lim.nconn * sizeof(uint32_t), 0xff}})) /* QTX_NO_POS */
        return e2;

    const ScanLevels R = scan_levels(tx->d_run_levels, n), S = scan_levels(tx->d_sent_levels, n);
    QuicTxArgs a{};
    a.conns = pr->d_conns;
    a.rx_phase = pr->d_rx_phase;
    a.reqs = d_reqs;
    a.n = (uint32_t)n;
    a.first = tx->d_first;
    a.runs = R.ref();
    a.nruns = R.total;
    a.sent = S.ref();
    a.run_start = tx->d_run_start;
    a.status = pr->d_status;
    a.pn_out = pr->d_pn_out;
    a.pkt_len = pr->d_pkt_len;
    a.pkt = static_cast<uint8_t *>(d_pkt);
    a.packed = tx->d_packed;
    a.recs = tx->d_recs;
    a.supp = tx->d_supp;
    a.keys = tx->d_keys;
    a.stats = tx->d_stats;
    const unsigned grid = quic_scan_grid((n + 255) / 256, eng->ncu);
    tx->sc.ev.mark(g_timing, 0, s);
    e = launch_quic_tx_heads(a, lim, grid, stream);
    if (e == 0)
        e = launch_scan_levels(R, eng->ncu, stream);
    if (e == 0)
        e = launch_quic_tx_runs(a, grid, stream);
    if (e == 0)
        e = launch_quic_tx_select(a, lim, grid, stream);
    if (e == 0)
        e = launch_scan_levels(S, eng->ncu, stream);
    if (e == 0)
        e = launch_quic_tx_build(a, lim, grid, stream);
    if (e == 0)
        e = launch_quic_tx_apply(a, lim, grid, stream);
    if (e != 0)
        return fail(PTLS_HIP_ELAUNCH, "%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)e));
    tx->sc.uses.note(stream);
    tx->sc.ev.mark(g_timing, 1, s);
    uint64_t st[QTX_NSTATS] = {};
    HIP_TRY(hipMemcpyAsync(st, tx->d_stats, sizeof(st), hipMemcpyDeviceToHost, s), PTLS_HIP_ENODEV);
    HIP_TRY(hipStreamSynchronize(s), PTLS_HIP_ENODEV);
    if (g_timing)
        g_front_ms = tx->sc.ev.between(0, 1), g_sort_ms = 0;
    const size_t m = (size_t)st[QTX_STAT_COUNT];
    report->n_sent = m;
    report->bytes = st[QTX_STAT_BYTES];
    tx->m = m;
    if (m == 0)
        return 0;

    LaunchPlan p{};
    p.eng = eng;
    p.n = m;
    p.d_recs = tx->d_recs;
    p.wg = WG_ALT;
    p.lanes = SPARSE_LANES;
    p.chacha_lanes = choose_chacha_lanes_from((double)st[QTX_STAT_BLOCKS64], m, (unsigned)eng->ncu); /* (below 2^53: exact) */
    p.all_aligned = false; /* packets lie at any byte offset */
    p.ncus = (unsigned)eng->ncu;
    if (!chacha) {
        /* the wave-per-record kernel's plan: a stable order by decreasing 16-byte block count, two radix digits of the key */
        tx->sc.ev.mark(g_timing, 2, s);
        e = tx->plan.sort(tx->d_keys, (uint32_t)m, eng->ncu, stream);
        if (e == 0)
            e = launch_quic_tx_order(tx->d_recs, tx->plan.d_order, (uint32_t)m, tx->d_recs_ord, tx->d_chunk, quic_scan_grid((m + 255) / 256, eng->ncu),
                                     stream);
        if (e != 0)
            return fail(PTLS_HIP_ELAUNCH, "%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)e));
        tx->sc.ev.mark(g_timing, 3, s);
        p.d_recs_ord = tx->d_recs_ord;
        p.d_order = tx->plan.d_order;
        p.d_chunks = tx->d_chunk;
        p.nchunks = 1;
    }
    /* the record (AAD = the unprotected header the build pass wrote into the packet) and the mask of its sample, then the header */
    if (int rc = run_plan(p, ks, d_in, d_pkt, d_pkt, nullptr, stream, false, hp_ks, tx->d_supp, tx->d_mask))
        return rc;
    e = quic_protect(tx->d_packed, m, d_pkt, tx->d_mask, stream);
    if (e != 0)
        return fail(PTLS_HIP_ELAUNCH, "%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)e));
    tx->sc.uses.note(stream);
    if (!chacha && tx->sc.ev.reached(g_timing, 3)) /* (a diagnostic: it waits for the sort, not for the record kernel) */
        g_sort_ms = tx->sc.ev.between(2, 3);
    report->lanes = chacha ? p.chacha_lanes : SPARSE_LANES;
    return 0;
}
