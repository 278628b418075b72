/*
 * quic_scratch.cpp -- what every QUIC device object shares on the host (quic_scratch.h): the scan levels, the owner of an
 * object's device arrays and timing events, the plan sort (quic_rx_kernel.hip's radix passes), the two-keyset refusals.
 */
#include <algorithm>

#include "host.h"

#define GF128_FN static inline
#include "quic_rx.h" /* (the sort key's digits) */

/* ---- the scan levels ---- */
unsigned quic_scan_grid(size_t items, int ncu)
{
    const size_t cap = (size_t)ncu * 8;
    return (unsigned)std::max<size_t>(1, std::min(items, cap));
}

/* the scan levels in one allocation: the counts, the span sums, their span sums, and the total */
ScanLevels scan_levels(uint32_t *base, size_t n)
{
    ScanLevels L{};
    L.n = n;
    L.n1 = (n + QP_SCAN_SPAN - 1) / QP_SCAN_SPAN;
    L.n2 = (L.n1 + QP_SCAN_SPAN - 1) / QP_SCAN_SPAN;
    L.has1 = L.n1 > 1, L.has2 = L.n2 > 1; /* n2 <= QP_SCAN_SPAN: n < 2^32 */
    const auto pad4 = [](size_t k) { return (k + 3) & ~(size_t)3; };
    const size_t o1 = pad4(n), o2 = o1 + pad4(L.has1 ? L.n1 : 0), ot = o2 + pad4(L.has2 ? L.n2 : 0);
    L.words = ot + 4;
    L.l0 = base;
    L.l1 = base + o1;
    L.l2 = base + o2;
    L.total = base + ot;
    return L;
}

/* one scan launch per level; the top level is a single span whose sum is the total */
int launch_scan_levels(const ScanLevels &L, int ncu, void *stream)
{
    int e = launch_quic_parse_scan(L.l0, (uint32_t)L.n, L.has1 ? L.l1 : L.total, quic_scan_grid(L.n1, ncu), stream);
    if (e == 0 && L.has1)
        e = launch_quic_parse_scan(L.l1, (uint32_t)L.n1, L.has2 ? L.l2 : L.total, quic_scan_grid(L.n2, ncu), stream);
    if (e == 0 && L.has2)
        e = launch_quic_parse_scan(L.l2, (uint32_t)L.n2, L.total, 1, stream);
    return e;
}

/* ---- timing events ---- */
void TimingEvents::destroy()
{
    for (hipEvent_t &e : ev) /* (those past `count` stay null) */
        if (e != nullptr) {
            (void)hipEventDestroy(e);
            e = nullptr;
        }
}

void TimingEvents::mark(bool on, int k, hipStream_t s)
{
    if (on && k < count && (ev[k] != nullptr || hipEventCreate(&ev[k]) == hipSuccess))
        (void)hipEventRecord(ev[k], s);
}

float TimingEvents::between(int a, int b) const
{
    float ms = 0;
    if (ev[a] == nullptr || ev[b] == nullptr || hipEventElapsedTime(&ms, ev[a], ev[b]) != hipSuccess)
        return 0;
    return ms;
}

bool TimingEvents::reached(bool on, int k) const
{
    if (!on || ev[k] == nullptr)
        return false;
    (void)hipEventSynchronize(ev[k]);
    return true;
}

/* ---- the owner of an object's device arrays ---- */
int DeviceScratch::ensure_bytes(void **p, size_t bytes)
{
    if (*p != nullptr)
        return 0;
    if (n_owned == MAX_ARRAYS)
        return fail(PTLS_HIP_ENOMEM, "%s: more than %zu device arrays in one object", prefix, MAX_ARRAYS);
    bytes = (bytes + 15) & ~(size_t)15;
    if (dev_alloc(eng, p, bytes) != hipSuccess)
        return fail(PTLS_HIP_ENOMEM, "%s: cannot allocate %zu bytes of device memory", prefix, bytes);
    owned[n_owned++] = *p;
    return 0;
}

int DeviceScratch::ensure_all(std::initializer_list<GrownArray> arrays)
{
    for (const GrownArray &a : arrays)
        if (int e = ensure_bytes(a.p, a.bytes))
            return e;
    return 0;
}

int DeviceScratch::grow(size_t *cap, size_t need, hipStream_t s, std::initializer_list<GrownArray> arrays)
{
    if (need <= *cap)
        return 0;
    if (std::any_of(arrays.begin(), arrays.end(), [](const GrownArray &a) { return *a.p != nullptr; })) {
        uses.wait(); /* the launches that used the smaller arrays */
        for (const GrownArray &a : arrays) {
            dev_free(eng, *a.p);
            n_owned = std::remove(owned, owned + n_owned, *a.p) - owned;
            *a.p = nullptr;
        }
        *cap = 0;
    }
    if (int e = ensure_all(arrays))
        return e;
    for (const GrownArray &a : arrays)
        if (a.fill >= 0)
            HIP_TRY(hipMemsetAsync(*a.p, a.fill, a.bytes, s), PTLS_HIP_ENODEV);
    *cap = need;
    return 0;
}

void DeviceScratch::release()
{
    if (n_owned == 0)
        return;
    DeviceGuard g(eng->device);
    uses.wait();
    while (n_owned != 0)
        dev_free(eng, owned[--n_owned]);
    ev.destroy();
    (void)hipStreamSynchronize(eng->util);
}

/* ---- the plan sort ---- */
static size_t sort_tiles(size_t m)
{
    return (m + QRX_TILE - 1) / QRX_TILE;
}

int PlanSort::ensure(DeviceScratch &sc, size_t cap, hipStream_t s)
{
    const bool fresh = d_order == nullptr;
    int e = sc.ensure(&d_order, cap * sizeof(uint32_t));
    if (e == 0)
        e = sc.ensure(&d_order_tmp, cap * sizeof(uint32_t));
    if (e == 0 && fresh) { /* once */
        HIP_TRY(hipMemsetAsync(d_order, 0, cap * sizeof(uint32_t), s), PTLS_HIP_ENODEV);
        HIP_TRY(hipMemsetAsync(d_order_tmp, 0, cap * sizeof(uint32_t), s), PTLS_HIP_ENODEV);
    }
    if (e == 0)
        e = sc.ensure(&d_hist, scan_levels(nullptr, QRX_DIGITS * sort_tiles(cap)).words * sizeof(uint32_t));
    return e;
}

/* one stable radix pass over m positions: counts, their scan, placement */
static int radix_pass(const PlanSort &ps, const uint32_t *d_keys, const uint32_t *src, uint32_t m, uint32_t shift, uint32_t *dst, int ncu,
                      void *stream)
{
    const ScanLevels H = scan_levels(ps.d_hist, QRX_DIGITS * sort_tiles(m));
    const ScanRef h = H.ref();
    int e = launch_quic_rx_hist(d_keys, src, m, shift, H.l0, stream);
    if (e == 0)
        e = launch_scan_levels(H, ncu, stream);
    if (e == 0)
        e = launch_quic_rx_scatter(d_keys, src, m, shift, h.l0, h.l1, h.l2, dst, stream);
    return e;
}

int PlanSort::sort(const uint32_t *d_keys, uint32_t m, int ncu, void *stream)
{
    int e = radix_pass(*this, d_keys, nullptr, m, 0, d_order_tmp, ncu, stream);
    if (e == 0)
        e = radix_pass(*this, d_keys, d_order_tmp, m, QRX_DIGIT_BITS, d_order, ncu, stream);
    return e;
}

/* ---- refusals ---- */
int quic_keysets_check(const char *who, const char *object, const ptls_hip_engine_t *eng, const ptls_hip_keyset_t *ks,
                       const ptls_hip_keyset_t *hp_ks, size_t stride)
{
    if (ks->eng != eng || hp_ks->eng != eng)
        return fail(PTLS_HIP_EINVAL, "%s: %s and keysets must belong to the same engine", who, object);
    if (hp_ks->algo != ks->algo || hp_ks->key_size != ks->key_size)
        return fail(PTLS_HIP_EINVAL, "%s: the header-protection keyset must be of the AEAD keyset's algorithm and key size", who);
    if (stride > ks->nslots / 3) /* (3 * stride <= nslots, without the product) */
        return fail(PTLS_HIP_EINVAL, "%s: three banks of stride %zu do not fit the keyset's %zu slots", who, stride, ks->nslots);
    return 0;
}

int quic_overlap_check(const char *who, const char *a_name, const void *a, size_t a_len, const char *b_name, const void *b,
                       size_t b_len)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    if (a_len != 0 && b_len != 0 && x < y + b_len && y < x + a_len)
        return fail(PTLS_HIP_EINVAL, "%s: the %s overlaps the %s", who, a_name, b_name);
    return 0;
}
