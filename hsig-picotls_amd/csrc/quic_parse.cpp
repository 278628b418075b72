/*
 * quic_parse.cpp -- QUIC datagrams parsed on the device (include/ptls_hip.h 2h): the connection-ID map (the
 * authoritative host mirror, its backward-shift removal, the upload of what changed) and the parse call (the host-side
 * refusals, the count / scan / write launches of quic_parse_kernel.hip, the copies back).  The hash, the probe loop and the
 * walk are quic_parse.h's, shared with the kernels.
 */
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <set>
#include <string>

#include "host.h"

#define GF128_FN static inline
#include "quic_parse.h"

static_assert(QP_INITIAL == PTLS_HIP_QUIC_TYPE_INITIAL && QP_ZERO_RTT == PTLS_HIP_QUIC_TYPE_ZERO_RTT &&
                  QP_HANDSHAKE == PTLS_HIP_QUIC_TYPE_HANDSHAKE && QP_RETRY == PTLS_HIP_QUIC_TYPE_RETRY &&
                  QP_ONE_RTT == PTLS_HIP_QUIC_TYPE_ONE_RTT && QP_VERSION_NEGOTIATION == PTLS_HIP_QUIC_TYPE_VERSION_NEGOTIATION &&
                  QP_UNKNOWN_VERSION == PTLS_HIP_QUIC_TYPE_UNKNOWN_VERSION && QP_NONE == PTLS_HIP_QUIC_TYPE_NONE,
              "quic_parse.h and ptls_hip.h name the same packet types");
static_assert(QP_OK == PTLS_HIP_QUIC_STATUS_OK && QP_TRUNCATED == PTLS_HIP_QUIC_STATUS_TRUNCATED &&
                  QP_TOO_SHORT == PTLS_HIP_QUIC_STATUS_TOO_SHORT && QP_BAD_CID_LEN == PTLS_HIP_QUIC_STATUS_BAD_CID_LEN &&
                  QP_BAD_FIXED_BIT == PTLS_HIP_QUIC_STATUS_BAD_FIXED_BIT && QP_NO_CONN == PTLS_HIP_QUIC_NO_CONN,
              "quic_parse.h and ptls_hip.h name the same statuses");
static_assert(sizeof(ptls_hip_quic_datagram_t) == 16 && sizeof(ptls_hip_quic_pktinfo_t) == 32 && sizeof(ptls_hip_quic_packet_t) == 40,
              "the layouts of include/ptls_hip.h 2e / 2h");

constexpr size_t CID_STRIDE = 20;
/* up to this many changed entries travel one by one; more, and the whole table is uploaded */
constexpr size_t CID_UPLOAD_SINGLY = 64;

struct st_ptls_hip_quic_cidmap_t {
    ptls_hip_engine_t *eng = nullptr;
    size_t capacity = 0, count = 0;
    std::vector<QuicCidEntry> table;   /* the authoritative mirror; size() = a power of two >= 2 * capacity */
    QuicCidEntry *d_table = nullptr;   /* allocated with the first upload (map_upload) */
    Uses uses;                         /* the parse launches that read d_table: updates and cidmap_free wait for them */
};

extern "C" ptls_hip_quic_cidmap_t *ptls_hip_quic_cidmap_new(ptls_hip_engine_t *eng, size_t capacity)
{
    if (eng == nullptr || capacity < 1 || capacity > ((size_t)1 << 30)) {
        fail(PTLS_HIP_EINVAL, "quic_cidmap_new: null engine, or capacity %zu outside 1 .. 2^30", capacity);
        return nullptr;
    }
    size_t size = 2;
    while (size < 2 * capacity)
        size <<= 1;
    auto *m = new st_ptls_hip_quic_cidmap_t();
    m->eng = eng;
    m->capacity = capacity;
    m->table.assign(size, QuicCidEntry{});
    return m;
}

extern "C" void ptls_hip_quic_cidmap_free(ptls_hip_quic_cidmap_t *m)
{
    if (m == nullptr)
        return;
    if (m->d_table != nullptr) {
        DeviceGuard g(m->eng->device);
        m->uses.wait();
        dev_free(m->eng, m->d_table);
    }
    delete m;
}

extern "C" size_t ptls_hip_quic_cidmap_size(ptls_hip_quic_cidmap_t *m)
{
    return m != nullptr ? m->count : 0;
}

/* the device table follows the mirror: the entries in `dirty`, or everything (also the first time); synchronous */
static int map_upload(const char *who, ptls_hip_quic_cidmap_t *m, const std::vector<uint32_t> *dirty, void *stream)
{
    DeviceGuard g(m->eng->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    bool whole = dirty == nullptr || dirty->size() > CID_UPLOAD_SINGLY;
    if (m->d_table == nullptr) {
        if (dev_alloc(m->eng, reinterpret_cast<void **>(&m->d_table), m->table.size() * sizeof(QuicCidEntry)) != hipSuccess)
            return fail(PTLS_HIP_ENOMEM, "%s: cannot allocate the table of %zu entries", who, m->table.size());
        whole = true;
    }
    m->uses.wait(); /* no parse launch still reads the entries about to change */
    if (whole) {
        HIP_TRY(hipMemcpyAsync(m->d_table, m->table.data(), m->table.size() * sizeof(QuicCidEntry), hipMemcpyHostToDevice, s),
                PTLS_HIP_ENODEV);
    } else {
        for (uint32_t i : *dirty)
            HIP_TRY(hipMemcpyAsync(m->d_table + i, &m->table[i], sizeof(QuicCidEntry), hipMemcpyHostToDevice, s), PTLS_HIP_ENODEV);
    }
    HIP_TRY(hipStreamSynchronize(s), PTLS_HIP_ENODEV);
    return 0;
}

static int map_check_keys(const char *who, ptls_hip_quic_cidmap_t *m, size_t count, const void *cids, const uint8_t *cid_lens)
{
    if (m == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null map", who);
    if (count != 0 && (cids == nullptr || cid_lens == nullptr))
        return fail(PTLS_HIP_EINVAL, "%s: null connection IDs or lengths", who);
    for (size_t i = 0; i < count; ++i)
        if (cid_lens[i] > QP_MAX_CID)
            return fail(PTLS_HIP_EINVAL, "%s: cid_lens[%zu] is %u, above 20", who, i, (unsigned)cid_lens[i]);
    return 0;
}

extern "C" int ptls_hip_quic_cidmap_set(ptls_hip_quic_cidmap_t *m, size_t count, const void *cids, const uint8_t *cid_lens,
                                        const uint32_t *conns, void *stream)
{
    const char *who = "quic_cidmap_set";
    if (int rc = map_check_keys(who, m, count, cids, cid_lens))
        return rc;
    if (count != 0 && conns == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null connection numbers", who);
    const uint8_t *c = static_cast<const uint8_t *>(cids);
    const uint32_t size = (uint32_t)m->table.size();
    /* nothing changes unless everything fits: the CIDs of the call that the map does not hold yet, each counted once */
    std::set<std::string> fresh;
    for (size_t i = 0; i < count; ++i) {
        if (conns[i] == QP_NO_CONN)
            return fail(PTLS_HIP_EINVAL, "%s: conns[%zu] is 0xffffffff, the value that means no connection", who, i);
        uint32_t slot;
        if (!quic_cid_probe(m->table.data(), size, c + i * CID_STRIDE, cid_lens[i], &slot))
            fresh.insert(std::string(reinterpret_cast<const char *>(c + i * CID_STRIDE), cid_lens[i]));
    }
    if (m->count + fresh.size() > m->capacity)
        return fail(PTLS_HIP_EINVAL, "%s: %zu connection IDs and %zu new ones exceed the capacity of %zu", who, m->count,
                    fresh.size(), m->capacity);
    if (count == 0)
        return 0;
    std::vector<uint32_t> dirty;
    const auto touched = [&dirty](uint32_t slot) { dirty.push_back(slot); };
    for (size_t i = 0; i < count; ++i) /* (a free entry exists: the load stays at or below 0.5) */
        if (quic_cid_set(m->table.data(), size, c + i * CID_STRIDE, cid_lens[i], conns[i], touched))
            ++m->count;
    return map_upload(who, m, &dirty, stream);
}

extern "C" int ptls_hip_quic_cidmap_remove(ptls_hip_quic_cidmap_t *m, size_t count, const void *cids, const uint8_t *cid_lens,
                                           void *stream)
{
    const char *who = "quic_cidmap_remove";
    if (int rc = map_check_keys(who, m, count, cids, cid_lens))
        return rc;
    const uint8_t *c = static_cast<const uint8_t *>(cids);
    const uint32_t size = (uint32_t)m->table.size();
    std::vector<uint32_t> dirty;
    const auto touched = [&dirty](uint32_t slot) { dirty.push_back(slot); };
    for (size_t i = 0; i < count; ++i)
        if (quic_cid_remove(m->table.data(), size, c + i * CID_STRIDE, cid_lens[i], touched))
            --m->count;
    if (dirty.empty())
        return 0;
    return map_upload(who, m, &dirty, stream);
}

/* ---- the parse call ---- */

static thread_local bool g_timing = false;
static thread_local float g_kernels_ms = 0, g_d2h_ms = 0;

extern "C" void ptls_hip_quic_parse_timing(int enable, float *kernels_ms, float *d2h_ms)
{
    g_timing = enable != 0;
    if (kernels_ms != nullptr)
        *kernels_ms = g_kernels_ms;
    if (d2h_ms != nullptr)
        *d2h_ms = g_d2h_ms;
}

namespace {

/* the device memory and the timing events of one call, released on every way out */
struct ParseScratch {
    ptls_hip_engine_t *eng;
    void *d_dgrams = nullptr, *d_levels = nullptr, *d_pkts = nullptr, *d_info = nullptr;
    TimingEvents ev{5};
    explicit ParseScratch(ptls_hip_engine_t *e) : eng(e) {}
    ~ParseScratch()
    {
        dev_free(eng, d_dgrams);
        dev_free(eng, d_levels);
        dev_free(eng, d_pkts);
        dev_free(eng, d_info);
    }
};

} // namespace

int quic_parse_check(const char *who, ptls_hip_engine_t *eng, const ptls_hip_quic_parse_params_t *pr, ptls_hip_quic_cidmap_t *map,
                     const ptls_hip_quic_datagram_t *dgrams, size_t n, size_t buf_len)
{
    if (pr->short_cid_len > QP_MAX_CID)
        return fail(PTLS_HIP_EINVAL, "%s: short_cid_len %u is above 20", who, pr->short_cid_len);
    if (pr->max_per_dgram < 1 || pr->max_per_dgram > 16)
        return fail(PTLS_HIP_EINVAL, "%s: max_per_dgram %u is outside 1..16", who, pr->max_per_dgram);
    if (pr->reserved != 0)
        return fail(PTLS_HIP_EINVAL, "%s: params.reserved must be 0", who);
    if (n > 0xffffffffu || n * (uint64_t)pr->max_per_dgram > 0xffffffffu)
        return fail(PTLS_HIP_EINVAL, "%s: %zu datagrams of up to %u entries are above 2^32 - 1", who, n, pr->max_per_dgram);
    if (map != nullptr && map->eng != eng)
        return fail(PTLS_HIP_EINVAL, "%s: the connection-ID map belongs to another engine", who);
    for (size_t i = 0; i < n; ++i) {
        if (dgrams[i].len > 65535)
            return fail(PTLS_HIP_EINVAL, "%s: datagram %zu: len %u is above 65535", who, i, dgrams[i].len);
        if (dgrams[i].off > buf_len || dgrams[i].len > buf_len - dgrams[i].off)
            return fail(PTLS_HIP_EINVAL, "%s: datagram %zu: off %llu + len %u is past the buffer of %zu bytes", who, i,
                        (unsigned long long)dgrams[i].off, dgrams[i].len, buf_len);
    }
    return 0;
}

int quic_parse_count(const char *who, ptls_hip_engine_t *eng, const ptls_hip_quic_parse_params_t *pr, ptls_hip_quic_cidmap_t *map,
                     const ptls_hip_quic_datagram_t *dgrams, size_t n, const void *d_buf, void *d_dgrams, uint32_t *d_levels,
                     void *stream, QuicParseArgs &a, unsigned *walk_grid, uint32_t *total, const std::function<void(int)> &mark)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (map != nullptr && map->d_table == nullptr) /* a map nothing was ever set in: the empty table */
        if (int rc = map_upload(who, map, nullptr, stream))
            return rc;
    const ScanLevels L = scan_levels(d_levels, n);
    a = QuicParseArgs{};
    a.dgrams = static_cast<const ptls_hip_quic_datagram_t *>(d_dgrams);
    a.n = (uint32_t)n;
    a.short_cid_len = pr->short_cid_len;
    a.max_per_dgram = pr->max_per_dgram;
    a.require_fixed_bit = pr->require_fixed_bit;
    a.buf = static_cast<const uint8_t *>(d_buf);
    a.scan = L.ref();
    a.table = map != nullptr ? map->d_table : nullptr;
    a.table_size = map != nullptr ? (uint32_t)map->table.size() : 0;
    a.expected_pn = pr->d_expected_pn;
    a.expected_count = pr->expected_count;
    *walk_grid = quic_scan_grid((n + 255) / 256, eng->ncu);

    mark(0);
    HIP_TRY(hipMemcpyAsync(d_dgrams, dgrams, n * sizeof(ptls_hip_quic_datagram_t), hipMemcpyHostToDevice, s), PTLS_HIP_ENODEV);
    int e = launch_quic_parse_count(a, *walk_grid, stream);
    if (e == 0)
        e = launch_scan_levels(L, eng->ncu, stream);
    if (e != 0)
        return fail(PTLS_HIP_ELAUNCH, "%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)e));
    if (map != nullptr)
        map->uses.note(stream);
    mark(1);
    *total = 0;
    HIP_TRY(hipMemcpyAsync(total, L.total, sizeof(*total), hipMemcpyDeviceToHost, s), PTLS_HIP_ENODEV);
    HIP_TRY(hipStreamSynchronize(s), PTLS_HIP_ENODEV);
    return 0;
}

int quic_parse_write(const char *who, ptls_hip_quic_cidmap_t *map, QuicParseArgs &a, unsigned walk_grid, ptls_hip_quic_packet_t *d_pkts,
                     ptls_hip_quic_pktinfo_t *d_info, void *stream)
{
    a.pkts = d_pkts;
    a.info = d_info;
    const int e = launch_quic_parse_write(a, walk_grid, stream);
    if (e != 0)
        return fail(PTLS_HIP_ELAUNCH, "%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)e));
    if (map != nullptr)
        map->uses.note(stream);
    return 0;
}

extern "C" int ptls_hip_quic_parse_datagrams(ptls_hip_engine_t *eng, const ptls_hip_quic_parse_params_t *pr,
                                             ptls_hip_quic_cidmap_t *map, const ptls_hip_quic_datagram_t *dgrams, size_t n,
                                             const void *d_buf, size_t buf_len, ptls_hip_quic_packet_t *h_pkts,
                                             ptls_hip_quic_pktinfo_t *h_info, size_t cap, size_t *n_pkts, void *stream)
{
    const char *who = "quic_parse_datagrams";
    if (eng == nullptr || pr == nullptr || n_pkts == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null engine, parameters or n_pkts", who);
    if (n != 0 && (dgrams == nullptr || d_buf == nullptr))
        return fail(PTLS_HIP_EINVAL, "%s: null datagram array or buffer", who);
    if (cap != 0 && (h_pkts == nullptr || h_info == nullptr))
        return fail(PTLS_HIP_EINVAL, "%s: null output array", who);
    if (int rc = quic_parse_check(who, eng, pr, map, dgrams, n, buf_len))
        return rc;
    if (n == 0) {
        *n_pkts = 0;
        return 0;
    }

    DeviceGuard g(eng->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    ParseScratch sc(eng);
    HIP_TRY(dev_alloc(eng, &sc.d_dgrams, n * sizeof(ptls_hip_quic_datagram_t)), PTLS_HIP_ENOMEM);
    HIP_TRY(dev_alloc(eng, &sc.d_levels, scan_levels(nullptr, n).words * sizeof(uint32_t)), PTLS_HIP_ENOMEM);
    QuicParseArgs a{};
    unsigned walk_grid = 1;
    uint32_t total = 0;
    if (int rc = quic_parse_count(who, eng, pr, map, dgrams, n, d_buf, sc.d_dgrams, static_cast<uint32_t *>(sc.d_levels), stream, a,
                                  &walk_grid, &total, [&](int k) { sc.ev.mark(g_timing, k, s); }))
        return rc;
    if (total > cap) {
        *n_pkts = total;
        return fail(PTLS_HIP_EINVAL, "%s: %u entries do not fit the arrays of %zu", who, total, cap);
    }
    if (total != 0) {
        HIP_TRY(dev_alloc(eng, &sc.d_pkts, (size_t)total * sizeof(ptls_hip_quic_packet_t)), PTLS_HIP_ENOMEM);
        HIP_TRY(dev_alloc(eng, &sc.d_info, (size_t)total * sizeof(ptls_hip_quic_pktinfo_t)), PTLS_HIP_ENOMEM);
        sc.ev.mark(g_timing, 2, s);
        if (int rc = quic_parse_write(who, map, a, walk_grid, static_cast<ptls_hip_quic_packet_t *>(sc.d_pkts),
                                      static_cast<ptls_hip_quic_pktinfo_t *>(sc.d_info), stream))
            return rc;
        sc.ev.mark(g_timing, 3, s);
        HIP_TRY(hipMemcpyAsync(h_pkts, sc.d_pkts, (size_t)total * sizeof(ptls_hip_quic_packet_t), hipMemcpyDeviceToHost, s),
                PTLS_HIP_ENODEV);
        HIP_TRY(hipMemcpyAsync(h_info, sc.d_info, (size_t)total * sizeof(ptls_hip_quic_pktinfo_t), hipMemcpyDeviceToHost, s),
                PTLS_HIP_ENODEV);
        sc.ev.mark(g_timing, 4, s);
        HIP_TRY(hipStreamSynchronize(s), PTLS_HIP_ENODEV);
    }
    if (g_timing) {
        /* kernels: the upload of the datagram array, count and scans (up to the host's look at the total), and the write pass */
        g_kernels_ms = sc.ev.between(0, 1) + sc.ev.between(2, 3);
        g_d2h_ms = sc.ev.between(3, 4);
    }
    *n_pkts = total;
    return 0;
}
