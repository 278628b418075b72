/*
 * quic_rx.cpp -- the receive object (include/ptls_hip.h 2i): parsed entries that stay on the device, and the
 * open call that selects, packs and plans them there and strings the existing header and record kernels behind: the host
 * sees the number of entries, five sums per open call, and nothing per packet.  The parse steps are quic_parse.cpp's, the
 * select rule and the sums' terms quic_rx.h's (shared with quic_rx_kernel.hip), the lane rules planner.cpp's, the record
 * launch batch.cpp's run_plan.  Where the planner wants the batch kernel (long key runs) the packed descriptors go back to
 * the host and through ptls_hip_quic_batch_new / ptls_hip_quic_open_batch as they are.
 * The same open call with the key chosen by Key Phase bit, and the commit of key updates (2j): the rule is
 * quic_phase.h's, the kernels quic_phase_kernel.hip's.
 * And the received packet numbers tracked behind an open call (2k): the rule is quic_track.h's, the kernels
 * quic_track_kernel.hip's.
 * And the ACK frames and send requests written from the tracked state (2m): the rule is quic_ack.h's, the
 * kernels quic_ack_kernel.hip's.
 */
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "host.h"

#define GF128_FN static inline
#include "quic_ack.h"
#include "quic_rx.h"
#include "quic_track.h"

namespace {

thread_local bool g_timing = false;
thread_local float g_select_ms = 0, g_plan_ms = 0, g_header_ms = 0, g_commit_ms = 0, g_track_ms = 0, g_ack_ms = 0;

} // namespace

struct st_ptls_hip_quic_rx_t {
    ptls_hip_engine_t *eng;
    size_t max_dgrams, cap;
    /* every d_ array below comes from here (rx_free: sc.release()); the timing events: select 0-1, sort 2-3, header kernel
     * 4-5, commit 6-7, track 8-9, ack 10-11 */
    DeviceScratch sc;
    size_t n = 0;          /* entries loaded */
    bool has_info = false; /* ... with info records */
    int mode = 0;          /* ptls_hip_quic_rx_set_plan */
    /* the entries, and the parse call's scratch (max_dgrams datagrams) */
    ptls_hip_quic_packet_t *d_pkts = nullptr;
    ptls_hip_quic_pktinfo_t *d_info = nullptr;
    void *d_dgrams = nullptr;
    uint32_t *d_parse_levels = nullptr;
    /* the open call's scratch (cap entries) */
    uint32_t *d_sel_levels = nullptr; /* the select flags and their scan */
    ptls_hip_quic_packet_t *d_packed = nullptr;
    uint32_t *d_keys = nullptr;
    ptls_hip_record_t *d_recs = nullptr, *d_recs_ord = nullptr;
    PlanSort plan;
    uint64_t *d_stats = nullptr;
    Chunk *d_chunk = nullptr;
    size_t order_n = 0; /* != 0: plan.d_order holds the last device-made AES plan order of that many packets */
    /* the commit's scratch (kp_cap connections): the two minima per connection, UINT64_MAX between calls; the scan levels */
    uint64_t *d_kp_mins = nullptr;
    uint32_t *d_kp_levels = nullptr;
    size_t kp_cap = 0;
    bool kp_open = false; /* the last open call was rx_open_keyphase: d_packed holds its kp_m selected packets */
    size_t kp_m = 0;
    /* the track call's scratch: per space the maximum and the window bits (tk_cap connections, 0 between calls), the scan
     * levels, and the table of candidates (tk_slots positions) */
    uint64_t *d_tk_acc = nullptr;
    uint32_t *d_tk_levels = nullptr, *d_tk_table = nullptr;
    size_t tk_cap = 0, tk_slots = 0;
    /* the ack call's scratch, one array (ak_cap list entries): the scan levels over the frame lengths, those over the "has a
     * frame" flags, and the two sums */
    uint32_t *d_ak_levels = nullptr;
    size_t ak_cap = 0;
    bool opened = false; /* an open call has run since the entries were loaded: d_packed holds its open_m selected packets */
    size_t open_m = 0;

    st_ptls_hip_quic_rx_t(ptls_hip_engine_t *e, size_t dgrams, size_t c) : eng(e), max_dgrams(dgrams), cap(c), sc(e, "quic_rx", 12) {}
    int ensure_entries()
    {
        if (int e = sc.ensure(&d_pkts, cap * sizeof(ptls_hip_quic_packet_t)))
            return e;
        return sc.ensure(&d_info, cap * sizeof(ptls_hip_quic_pktinfo_t));
    }
};

extern "C" ptls_hip_quic_rx_t *ptls_hip_quic_rx_new(ptls_hip_engine_t *eng, size_t max_dgrams, size_t cap)
{
    if (eng == nullptr || cap < 1 || cap > 0xffffffffu || max_dgrams > 0xffffffffu) {
        fail(PTLS_HIP_EINVAL, "quic_rx_new: null engine, cap %zu outside 1 .. 2^32 - 1, or max_dgrams %zu above 2^32 - 1", cap,
             max_dgrams);
        return nullptr;
    }
    return new st_ptls_hip_quic_rx_t(eng, max_dgrams, cap); /* device memory comes with the first use of each array */
}

extern "C" void ptls_hip_quic_rx_free(ptls_hip_quic_rx_t *rx)
{
    if (rx == nullptr)
        return;
    rx->sc.release();
    delete rx;
}

extern "C" int ptls_hip_quic_rx_parse(ptls_hip_quic_rx_t *rx, const ptls_hip_quic_parse_params_t *pr, ptls_hip_quic_cidmap_t *map,
                                      const ptls_hip_quic_datagram_t *dgrams, size_t n, const void *d_buf, size_t buf_len,
                                      size_t *n_pkts, void *stream)
{
    const char *who = "quic_rx_parse";
    if (rx == nullptr || pr == nullptr || n_pkts == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null receive object, parameters or n_pkts", who);
    if (n != 0 && (dgrams == nullptr || d_buf == nullptr))
        return fail(PTLS_HIP_EINVAL, "%s: null datagram array or buffer", who);
    if (n > rx->max_dgrams)
        return fail(PTLS_HIP_EINVAL, "%s: %zu datagrams, the receive object was made for %zu", who, n, rx->max_dgrams);
    if (int rc = quic_parse_check(who, rx->eng, pr, map, dgrams, n, buf_len))
        return rc;
    rx->n = 0;
    rx->has_info = true;
    rx->order_n = 0;
    rx->kp_open = false;
    rx->opened = false;
    *n_pkts = 0;
    if (n == 0)
        return 0;

    ptls_hip_engine_t *eng = rx->eng;
    DeviceGuard g(eng->device);
    if (int e = rx->sc.ensure(&rx->d_dgrams, rx->max_dgrams * sizeof(ptls_hip_quic_datagram_t)))
        return e;
    if (int e = rx->sc.ensure(&rx->d_parse_levels, scan_levels(nullptr, rx->max_dgrams).words * sizeof(uint32_t)))
        return e;
    if (int e = rx->ensure_entries())
        return e;
    QuicParseArgs a{};
    unsigned walk_grid = 1;
    uint32_t total = 0;
    rx->sc.uses.note(stream);
    if (int rc = quic_parse_count(who, eng, pr, map, dgrams, n, d_buf, rx->d_dgrams, rx->d_parse_levels, stream, a, &walk_grid, &total,
                                  [](int) {}))
        return rc;
    if (total > rx->cap) {
        *n_pkts = total;
        return fail(PTLS_HIP_EINVAL, "%s: %u entries do not fit the receive object's %zu", who, total, rx->cap);
    }
    if (total != 0) {
        if (int rc = quic_parse_write(who, map, a, walk_grid, rx->d_pkts, rx->d_info, stream))
            return rc;
        rx->sc.uses.note(stream);
    }
    rx->n = total;
    *n_pkts = total;
    return 0;
}

extern "C" int ptls_hip_quic_rx_set_packets(ptls_hip_quic_rx_t *rx, const ptls_hip_quic_packet_t *d_pkts,
                                            const ptls_hip_quic_pktinfo_t *d_info, size_t n, void *stream)
{
    const char *who = "quic_rx_set_packets";
    if (rx == nullptr || (n != 0 && d_pkts == nullptr))
        return fail(PTLS_HIP_EINVAL, "%s: null receive object or descriptor array", who);
    if (n > rx->cap)
        return fail(PTLS_HIP_EINVAL, "%s: %zu descriptors, the receive object holds %zu", who, n, rx->cap);
    rx->n = 0;
    rx->has_info = d_info != nullptr;
    rx->order_n = 0;
    rx->kp_open = false;
    rx->opened = false;
    if (n == 0)
        return 0;
    DeviceGuard g(rx->eng->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int e = rx->ensure_entries())
        return e;
    HIP_TRY(hipMemcpyAsync(rx->d_pkts, d_pkts, n * sizeof(ptls_hip_quic_packet_t), hipMemcpyDeviceToDevice, s), PTLS_HIP_ENODEV);
    if (d_info != nullptr)
        HIP_TRY(hipMemcpyAsync(rx->d_info, d_info, n * sizeof(ptls_hip_quic_pktinfo_t), hipMemcpyDeviceToDevice, s), PTLS_HIP_ENODEV);
    rx->sc.uses.note(stream);
    rx->n = n;
    return 0;
}

extern "C" const ptls_hip_quic_packet_t *ptls_hip_quic_rx_packets(ptls_hip_quic_rx_t *rx)
{
    return rx != nullptr && rx->n != 0 ? rx->d_pkts : nullptr;
}

extern "C" const ptls_hip_quic_pktinfo_t *ptls_hip_quic_rx_info(ptls_hip_quic_rx_t *rx)
{
    return rx != nullptr && rx->n != 0 && rx->has_info ? rx->d_info : nullptr;
}

extern "C" size_t ptls_hip_quic_rx_count(ptls_hip_quic_rx_t *rx)
{
    return rx != nullptr ? rx->n : 0;
}

extern "C" int ptls_hip_quic_rx_set_plan(ptls_hip_quic_rx_t *rx, int mode)
{
    if (rx == nullptr || mode < 0 || mode > 2)
        return fail(PTLS_HIP_EINVAL, "quic_rx_set_plan: null receive object, or a mode other than 0 (auto), 1 (device) and 2 (host)");
    rx->mode = mode;
    return 0;
}

extern "C" const uint32_t *ptls_hip_quic_rx_order(ptls_hip_quic_rx_t *rx)
{
    return rx != nullptr && rx->order_n != 0 ? rx->plan.d_order : nullptr;
}

extern "C" void ptls_hip_quic_rx_timing(int enable, float *select_ms, float *plan_ms)
{
    g_timing = enable != 0;
    if (select_ms != nullptr)
        *select_ms = g_select_ms;
    if (plan_ms != nullptr)
        *plan_ms = g_plan_ms;
}

extern "C" void ptls_hip_quic_rx_keyphase_timing(float *header_ms, float *commit_ms)
{
    if (header_ms != nullptr)
        *header_ms = g_header_ms;
    if (commit_ms != nullptr)
        *commit_ms = g_commit_ms;
}

/* the packed descriptors back to the host and through the existing calls, planned there */
static int open_on_host(ptls_hip_quic_rx_t *rx, size_t m, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, void *d_buf, void *d_out,
                        uint64_t *d_result, uint64_t *d_pn_out, ptls_hip_quic_rx_report_t *report, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<ptls_hip_quic_packet_t> h(m);
    HIP_TRY(hipMemcpyAsync(h.data(), rx->d_packed, m * sizeof(ptls_hip_quic_packet_t), hipMemcpyDeviceToHost, s), PTLS_HIP_ENODEV);
    HIP_TRY(hipStreamSynchronize(s), PTLS_HIP_ENODEV);
    ptls_hip_quic_batch_t *q = ptls_hip_quic_batch_new(rx->eng, h.data(), m, 1, stream);
    if (q == nullptr)
        return PTLS_HIP_EINVAL; /* (the message is batch_new's) */
    int lanes = 0, chacha_lanes = 0;
    quic_batch_lanes(q, &lanes, &chacha_lanes);
    report->lanes = ks->algo == PTLS_HIP_ALGO_CHACHA20POLY1305 ? chacha_lanes : lanes;
    const int rc = ptls_hip_quic_open_batch(q, ks, hp_ks, d_buf, d_out, d_result, d_pn_out, stream);
    ptls_hip_quic_batch_free(q); /* waits for the launches */
    return rc;
}

/* both open calls; kp == nullptr: ptls_hip_quic_rx_open */
static int rx_open(const char *who, ptls_hip_quic_rx_t *rx, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, uint32_t type_mask,
                   const ptls_hip_quic_rx_keyphase_t *kp, void *d_buf, size_t buf_len, void *d_out, size_t out_len, uint32_t *d_sel,
                   uint64_t *d_result, uint64_t *d_pn_out, ptls_hip_quic_rx_report_t *report, void *stream)
{
    if (rx == nullptr || ks == nullptr || hp_ks == nullptr || report == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null receive object, keyset or report", who);
    if (kp != nullptr) {
        if (kp->d_phase == nullptr || kp->d_gen_out == nullptr)
            return fail(PTLS_HIP_EINVAL, "%s: null key-phase state or generation array", who);
        if (kp->stride == 0 || kp->count == 0)
            return fail(PTLS_HIP_EINVAL, "%s: a bank stride or a state count of 0", who);
        if (rx->mode == 2)
            return fail(PTLS_HIP_EINVAL, "%s: the host plan (rx_set_plan 2) fixes a chunk's key on the host", who);
    }
    if (int rc = quic_keysets_check(who, "receive object", rx->eng, ks, hp_ks, kp != nullptr ? kp->stride : 0))
        return rc;
    report->n_selected = 0;
    report->planned_on_device = 0;
    report->lanes = 0;
    rx->kp_open = false;
    rx->opened = false;
    if (rx->n == 0)
        return 0;
    if (d_buf == nullptr || d_out == nullptr || d_sel == nullptr || d_result == nullptr || d_pn_out == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null buffer", who);
    if (int rc = quic_overlap_check(who, "output buffer", d_out, out_len, "packet buffer", d_buf, buf_len))
        return rc;

    ptls_hip_engine_t *eng = rx->eng;
    DeviceGuard g(eng->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t cap = rx->cap;
    int e = rx->sc.ensure_all({{&rx->d_sel_levels, scan_levels(nullptr, cap).words * sizeof(uint32_t)},
                               {&rx->d_packed, cap * sizeof(ptls_hip_quic_packet_t)}, {&rx->d_keys, cap * sizeof(uint32_t)},
                               {&rx->d_recs, cap * sizeof(ptls_hip_record_t)}, {&rx->d_stats, QRX_NSTATS * sizeof(uint64_t)},
                               {&rx->d_chunk, sizeof(Chunk)}});
    if (e != 0)
        return e;
    rx->order_n = 0;

    /* select, scan, compact, stats: one readback of QRX_NSTATS sums is all the host learns of the packets */
    const ScanLevels L = scan_levels(rx->d_sel_levels, rx->n);
    QuicRxLimits lim{};
    lim.buf_len = buf_len;
    lim.out_len = out_len;
    lim.nslots = kp != nullptr ? std::min(kp->stride, kp->count) : ks->nslots; /* (the state is indexed by the key) */
    lim.hp_nslots = hp_ks->nslots;
    lim.type_mask = type_mask;
    lim.has_info = rx->has_info ? 1u : 0u;
    QuicRxArgs a{};
    a.pkts = rx->d_pkts;
    a.info = rx->has_info ? rx->d_info : nullptr;
    a.n = (uint32_t)rx->n;
    a.scan = L.ref();
    a.total = L.total;
    a.sel = d_sel;
    a.packed = rx->d_packed;
    a.keys = rx->d_keys;
    a.stats = rx->d_stats;
    a.chunk = rx->d_chunk;
    const unsigned grid = quic_scan_grid((rx->n + 255) / 256, eng->ncu);
    rx->sc.ev.mark(g_timing, 0, s);
    e = launch_quic_rx_select(a, lim, grid, stream);
    if (e == 0)
        e = launch_scan_levels(L, eng->ncu, stream);
    if (e == 0)
        e = launch_quic_rx_compact(a, lim, grid, stream);
    if (e == 0)
        e = launch_quic_rx_stats(a, grid, stream);
    if (e != 0)
        return fail(PTLS_HIP_ELAUNCH, "%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)e));
    rx->sc.uses.note(stream);
    rx->sc.ev.mark(g_timing, 1, s);
    uint64_t st[QRX_NSTATS] = {};
    HIP_TRY(hipMemcpyAsync(st, rx->d_stats, sizeof(st), hipMemcpyDeviceToHost, s), PTLS_HIP_ENODEV);
    HIP_TRY(hipStreamSynchronize(s), PTLS_HIP_ENODEV);
    if (g_timing)
        g_select_ms = rx->sc.ev.between(0, 1), g_plan_ms = 0;
    const size_t m = (size_t)st[QRX_STAT_COUNT];
    report->n_selected = m;
    rx->kp_open = kp != nullptr;
    rx->kp_m = m;
    rx->opened = true;
    rx->open_m = m;
    if (m == 0)
        return 0;

    /* the lanes, by the planner's rules from the sums (integers below 2^53: exact in a double) */
    const bool chacha = ks->algo == PTLS_HIP_ALGO_CHACHA20POLY1305;
    const int lanes = choose_lanes_from((double)st[QRX_STAT_GHASH], m, (size_t)st[QRX_STAT_RUNS] + 1, (unsigned)eng->ncu);
    const int chacha_lanes = choose_chacha_lanes_from((double)st[QRX_STAT_BLOCKS64], m, (unsigned)eng->ncu);
    /* with a key per record (kp) only the two kernels that read rec.key per record can run: always the device plan */
    const bool on_device = kp != nullptr || rx->mode == 1 || (rx->mode == 0 && (chacha || lanes == SPARSE_LANES));
    if (!on_device)
        return open_on_host(rx, m, ks, hp_ks, d_buf, d_out, d_result, d_pn_out, report, stream);

    LaunchPlan p{};
    p.eng = eng;
    p.n = m;
    p.d_recs = rx->d_recs;
    p.wg = WG_ALT;
    p.lanes = SPARSE_LANES;
    p.chacha_lanes = chacha_lanes;
    p.all_aligned = false; /* packets lie at any byte offset; the header kernel writes the real in_off */
    p.ncus = (unsigned)eng->ncu;
    if (!chacha) {
        /* the sparse kernel's plan: a stable order by decreasing 16-byte block count, two radix digits of the 12-bit key */
        e = rx->sc.ensure(&rx->d_recs_ord, cap * sizeof(ptls_hip_record_t));
        if (e == 0)
            e = rx->plan.ensure(rx->sc, cap, s);
        if (e != 0)
            return e;
        rx->sc.ev.mark(g_timing, 2, s);
        e = rx->plan.sort(rx->d_keys, (uint32_t)m, eng->ncu, stream);
        if (e != 0)
            return fail(PTLS_HIP_ELAUNCH, "%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)e));
        rx->sc.ev.mark(g_timing, 3, s);
        p.d_recs_ord = rx->d_recs_ord;
        p.d_order = rx->plan.d_order;
        p.d_chunks = rx->d_chunk;
        p.nchunks = 1;
    }
    QuicPhaseArgs ph{};
    if (kp != nullptr) {
        ph.phase = kp->d_phase;
        ph.stride = (uint32_t)kp->stride; /* 3 * stride <= nslots < 2^32 */
        ph.gen_out = kp->d_gen_out;
    }
    if (kp != nullptr)
        rx->sc.ev.mark(g_timing, 4, s);
    e = quic_unprotect(eng, hp_ks, rx->d_packed, m, p.d_recs, p.d_recs_ord, p.d_order, d_buf, d_pn_out, stream, /* (ChaCha: no order) */
                       kp != nullptr ? &ph : nullptr);
    if (e != 0)
        return fail(PTLS_HIP_ELAUNCH, "%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)e));
    if (kp != nullptr)
        rx->sc.ev.mark(g_timing, 5, s);
    keyset_note_use(hp_ks, stream);
    rx->sc.uses.note(stream);
    if (int rc = run_plan(p, ks, d_buf, d_buf, d_out, d_result, stream, true))
        return rc;
    rx->sc.uses.note(stream);
    if (!chacha)
        rx->order_n = m;
    if (!chacha && rx->sc.ev.reached(g_timing, 3)) /* (a diagnostic: it waits for the sort, not for the open kernel) */
        g_plan_ms = rx->sc.ev.between(2, 3);
    if (kp != nullptr && rx->sc.ev.reached(g_timing, 5)) /* (likewise: it waits for the header kernel) */
        g_header_ms = rx->sc.ev.between(4, 5);
    report->planned_on_device = 1;
    report->lanes = chacha ? chacha_lanes : SPARSE_LANES;
    return 0;
}

extern "C" int ptls_hip_quic_rx_open(ptls_hip_quic_rx_t *rx, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, uint32_t type_mask,
                                     void *d_buf, size_t buf_len, void *d_out, size_t out_len, uint32_t *d_sel, uint64_t *d_result,
                                     uint64_t *d_pn_out, ptls_hip_quic_rx_report_t *report, void *stream)
{
    return rx_open("quic_rx_open", rx, ks, hp_ks, type_mask, nullptr, d_buf, buf_len, d_out, out_len, d_sel, d_result, d_pn_out, report,
                   stream);
}

extern "C" int ptls_hip_quic_rx_open_keyphase(ptls_hip_quic_rx_t *rx, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                                              uint32_t type_mask, const ptls_hip_quic_rx_keyphase_t *kp, void *d_buf, size_t buf_len,
                                              void *d_out, size_t out_len, uint32_t *d_sel, uint64_t *d_result, uint64_t *d_pn_out,
                                              ptls_hip_quic_rx_report_t *report, void *stream)
{
    const char *who = "quic_rx_open_keyphase";
    if (kp == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null key-phase parameters", who);
    return rx_open(who, rx, ks, hp_ks, type_mask, kp, d_buf, buf_len, d_out, out_len, d_sel, d_result, d_pn_out, report, stream);
}

extern "C" int ptls_hip_quic_rx_keyphase_commit(ptls_hip_quic_rx_t *rx, ptls_hip_quic_keyphase_t *d_phase, size_t count,
                                                const uint64_t *d_result, const uint64_t *d_pn_out, const uint32_t *d_gen_out,
                                                uint32_t *d_updated, size_t *n_updated, void *stream)
{
    const char *who = "quic_rx_keyphase_commit";
    if (rx == nullptr || d_phase == nullptr || d_result == nullptr || d_pn_out == nullptr || d_gen_out == nullptr ||
        d_updated == nullptr || n_updated == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null receive object, state, array or n_updated", who);
    if (count == 0 || count > 0xffffffffu)
        return fail(PTLS_HIP_EINVAL, "%s: a state count of %zu is outside 1 .. 2^32 - 1", who, count);
    if (!rx->kp_open)
        return fail(PTLS_HIP_EINVAL, "%s: no rx_open_keyphase on the object since its entries were loaded or since a plain rx_open", who);
    *n_updated = 0;
    const size_t m = rx->kp_m;
    if (m == 0)
        return 0; /* nothing was selected: no entry changes */

    ptls_hip_engine_t *eng = rx->eng;
    DeviceGuard g(eng->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int e = rx->sc.grow(&rx->kp_cap, count, s, {{&rx->d_kp_mins, 2 * count * sizeof(uint64_t), 0xff}, /* UINT64_MAX */
                                                    {&rx->d_kp_levels, scan_levels(nullptr, count).words * sizeof(uint32_t)}}))
        return e;
    const ScanLevels L = scan_levels(rx->d_kp_levels, count);
    QuicCommitArgs a{};
    a.phase = d_phase;
    a.count = (uint32_t)count;
    a.packed = rx->d_packed;
    a.result = d_result;
    a.pn_out = d_pn_out;
    a.gen_out = d_gen_out;
    a.mins = rx->d_kp_mins;
    a.scan = L.ref();
    a.updated = d_updated;
    /* the mark pass: QPH_MARK_PER_THREAD packets per thread, so that a lane has successive packets to fold (internal.h) */
    const unsigned pkt_grid = quic_scan_grid((m + 256 * QPH_MARK_PER_THREAD - 1) / (256 * QPH_MARK_PER_THREAD), eng->ncu);
    const unsigned conn_grid = quic_scan_grid((count + 255) / 256, eng->ncu);
    rx->sc.ev.mark(g_timing, 6, s);
    int e = launch_quic_phase_mark(a, (uint32_t)m, pkt_grid, stream);
    if (e == 0)
        e = launch_quic_phase_apply(a, 0, conn_grid, stream);
    if (e == 0)
        e = launch_scan_levels(L, eng->ncu, stream);
    if (e == 0)
        e = launch_quic_phase_apply(a, 1, conn_grid, stream);
    if (e != 0)
        return fail(PTLS_HIP_ELAUNCH, "%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)e));
    rx->sc.uses.note(stream);
    rx->sc.ev.mark(g_timing, 7, s);
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, L.total, sizeof(total), hipMemcpyDeviceToHost, s), PTLS_HIP_ENODEV);
    HIP_TRY(hipStreamSynchronize(s), PTLS_HIP_ENODEV);
    if (g_timing)
        g_commit_ms = rx->sc.ev.between(6, 7);
    *n_updated = total;
    return 0;
}

extern "C" void ptls_hip_quic_rx_track_timing(float *track_ms)
{
    if (track_ms != nullptr)
        *track_ms = g_track_ms;
}

extern "C" int ptls_hip_quic_rx_track(ptls_hip_quic_rx_t *rx, const ptls_hip_quic_rx_track_t *tr, const uint32_t *d_sel,
                                      const uint64_t *d_result, const uint64_t *d_pn_out, size_t *n_touched, void *stream)
{
    const char *who = "quic_rx_track";
    if (rx == nullptr || tr == nullptr || d_sel == nullptr || d_result == nullptr || d_pn_out == nullptr || n_touched == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null receive object, parameters, array or n_touched", who);
    if (tr->d_spaces == nullptr || tr->d_verdict == nullptr || tr->d_touched == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null state, verdict or touched array", who);
    if (tr->count == 0 || tr->count > 0xffffffffu)
        return fail(PTLS_HIP_EINVAL, "%s: a connection count of %zu is outside 1 .. 2^32 - 1", who, tr->count);
    if (tr->d_expected_pn == nullptr && tr->expected_count != 0)
        return fail(PTLS_HIP_EINVAL, "%s: no expected-pn table, but %zu entries of it", who, tr->expected_count);
    if (!rx->opened)
        return fail(PTLS_HIP_EINVAL, "%s: no open call on the object since its entries were loaded", who);
    if (!rx->has_info)
        return fail(PTLS_HIP_EINVAL, "%s: the entries were loaded without info records: no packet-number space is known", who);
    *n_touched = 0;
    const size_t m = rx->open_m, count = tr->count;
    if (m == 0)
        return 0; /* nothing was selected: no entry changes */

    ptls_hip_engine_t *eng = rx->eng;
    DeviceGuard g(eng->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int e = rx->sc.grow(&rx->tk_cap, count, s, {{&rx->d_tk_acc, 6 * count * sizeof(uint64_t), 0},
                                                    {&rx->d_tk_levels, scan_levels(nullptr, count).words * sizeof(uint32_t)}}))
        return e;
    const uint64_t slots = quic_track_slots(m);
    if (int e = rx->sc.grow(&rx->tk_slots, slots, s, {{&rx->d_tk_table, slots * sizeof(uint32_t)}})) /* (filled per call, below) */
        return e;
    const ScanLevels L = scan_levels(rx->d_tk_levels, count);
    QuicTrackArgs a{};
    a.spaces = tr->d_spaces;
    a.count = (uint32_t)count;
    a.n = (uint32_t)rx->n;
    a.packed = rx->d_packed;
    a.info = rx->d_info;
    a.sel = d_sel;
    a.result = d_result;
    a.pn_out = d_pn_out;
    a.acc = rx->d_tk_acc;
    a.table = rx->d_tk_table;
    a.slots = slots;
    a.verdict = tr->d_verdict;
    a.expected_pn = tr->d_expected_pn;
    a.expected_count = tr->expected_count;
    a.scan = L.ref();
    a.touched = tr->d_touched;
    const unsigned claim_grid = quic_scan_grid((m + 256 * QTK_CLAIM_PER_THREAD - 1) / (256 * QTK_CLAIM_PER_THREAD), eng->ncu);
    const unsigned pkt_grid = quic_scan_grid((m + 255) / 256, eng->ncu);
    const unsigned conn_grid = quic_scan_grid((count + 255) / 256, eng->ncu);
    rx->sc.ev.mark(g_timing, 8, s);
    HIP_TRY(hipMemsetAsync(rx->d_tk_table, 0xff, slots * sizeof(uint32_t), s), PTLS_HIP_ENODEV); /* every slot QTK_EMPTY */
    int e = launch_quic_track_claim(a, (uint32_t)m, claim_grid, stream);
    if (e == 0)
        e = launch_quic_track_verdict(a, (uint32_t)m, pkt_grid, stream);
    if (e == 0)
        e = launch_quic_track_apply(a, 0, conn_grid, stream);
    if (e == 0)
        e = launch_scan_levels(L, eng->ncu, stream);
    if (e == 0)
        e = launch_quic_track_apply(a, 1, conn_grid, stream);
    if (e != 0)
        return fail(PTLS_HIP_ELAUNCH, "%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)e));
    rx->sc.uses.note(stream);
    rx->sc.ev.mark(g_timing, 9, s);
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, L.total, sizeof(total), hipMemcpyDeviceToHost, s), PTLS_HIP_ENODEV);
    HIP_TRY(hipStreamSynchronize(s), PTLS_HIP_ENODEV);
    if (g_timing)
        g_track_ms = rx->sc.ev.between(8, 9);
    *n_touched = total;
    return 0;
}

extern "C" void ptls_hip_quic_rx_ack_timing(float *ack_ms)
{
    if (ack_ms != nullptr)
        *ack_ms = g_ack_ms;
}

extern "C" int ptls_hip_quic_rx_ack(ptls_hip_quic_rx_t *rx, const ptls_hip_quic_rx_ack_t *pr, const uint32_t *d_list, size_t n,
                                    ptls_hip_quic_rx_ack_report_t *report, void *stream)
{
    const char *who = "quic_rx_ack";
    constexpr uint64_t MAX = PTLS_HIP_QUIC_ACK_MAX;
    if (rx == nullptr || pr == nullptr || report == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null receive object, parameters or report", who);
    if (pr->d_spaces == nullptr || pr->d_status == nullptr || pr->d_frame_off == nullptr || pr->d_frame_len == nullptr ||
        pr->d_reqs == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null state, status, frame-offset, frame-length or request array", who);
    if (n != 0 && (d_list == nullptr || pr->d_frames == nullptr))
        return fail(PTLS_HIP_EINVAL, "%s: null list or frame buffer", who);
    if (pr->count == 0 || pr->count > 0xffffffffu)
        return fail(PTLS_HIP_EINVAL, "%s: a connection count of %zu is outside 1 .. 2^32 - 1", who, pr->count);
    if (pr->space > 2)
        return fail(PTLS_HIP_EINVAL, "%s: packet-number space %u is above 2", who, pr->space);
    if (pr->ack_delay >= ptls_hip::QAK_VARINT_END)
        return fail(PTLS_HIP_EINVAL, "%s: an ack_delay of %llu is not below 2^62", who, (unsigned long long)pr->ack_delay);
    if (n > 0xffffffffu / MAX)
        return fail(PTLS_HIP_EINVAL, "%s: %zu list entries: 81 bytes each do not fit the 32-bit scan levels", who, n);
    if (pr->frames_len < MAX * n)
        return fail(PTLS_HIP_EINVAL, "%s: a frame buffer of %zu bytes is below 81 for each of the %zu list entries", who, pr->frames_len, n);
    if (pr->in_off > UINT64_MAX - MAX * n)
        return fail(PTLS_HIP_EINVAL, "%s: in_off plus 81 bytes for each of the %zu list entries wraps 2^64", who, n);
    if (pr->pkt_stride != 0 && n > (UINT64_MAX - pr->pkt_base) / pr->pkt_stride)
        return fail(PTLS_HIP_EINVAL, "%s: pkt_base plus %zu packets of stride %llu wraps 2^64", who, n, (unsigned long long)pr->pkt_stride);
    report->n_frames = 0;
    report->bytes = 0;
    if (n == 0)
        return 0;

    ptls_hip_engine_t *eng = rx->eng;
    DeviceGuard g(eng->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    /* (the words of n entries' levels grow with n: two sets of them and the sums fit what the capacity allocated) */
    if (int e = rx->sc.grow(&rx->ak_cap, n, s, {{&rx->d_ak_levels, (2 * scan_levels(nullptr, n).words + 4) * sizeof(uint32_t)}}))
        return e;
    const size_t words = scan_levels(nullptr, n).words; /* a multiple of 4: the sums behind both are 16-byte aligned */
    const ScanLevels Ll = scan_levels(rx->d_ak_levels, n), Lf = scan_levels(rx->d_ak_levels + words, n);
    uint64_t *d_sums = reinterpret_cast<uint64_t *>(rx->d_ak_levels + 2 * words);
    QuicAckArgs a{};
    a.spaces = pr->d_spaces;
    a.count = (uint32_t)pr->count;
    a.space = pr->space;
    a.list = d_list;
    a.n = (uint32_t)n;
    a.max_ranges = pr->max_ranges;
    a.ack_delay = pr->ack_delay;
    a.lens = Ll.ref();
    a.flags = Lf.ref();
    a.sums = d_sums;
    a.frames = static_cast<uint8_t *>(pr->d_frames);
    a.in_off = pr->in_off;
    a.pkt_base = pr->pkt_base;
    a.pkt_stride = pr->pkt_stride;
    a.status = pr->d_status;
    a.frame_off = pr->d_frame_off;
    a.frame_len = pr->d_frame_len;
    a.reqs = pr->d_reqs;
    const unsigned grid = quic_scan_grid((n + 255) / 256, eng->ncu);
    rx->sc.ev.mark(g_timing, 10, s);
    int e = launch_quic_ack_size(a, grid, stream);
    if (e == 0)
        e = launch_scan_levels(Ll, eng->ncu, stream);
    if (e == 0)
        e = launch_scan_levels(Lf, eng->ncu, stream);
    if (e == 0)
        e = launch_quic_ack_write(a, grid, stream);
    if (e != 0)
        return fail(PTLS_HIP_ELAUNCH, "%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)e));
    rx->sc.uses.note(stream);
    rx->sc.ev.mark(g_timing, 11, s);
    uint64_t sums[2] = {};
    HIP_TRY(hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, s), PTLS_HIP_ENODEV);
    HIP_TRY(hipStreamSynchronize(s), PTLS_HIP_ENODEV);
    if (g_timing)
        g_ack_ms = rx->sc.ev.between(10, 11);
    report->bytes = sums[0];
    report->n_frames = sums[1];
    return 0;
}
