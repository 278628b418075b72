/*
 * quic_track_kernel.hip -- received QUIC packet numbers tracked on the device: replays found, the per-space state and the
 * expected packet numbers moved on (include/ptls_hip.h 2k).  The rule is quic_track.h's.
 *
 *   quic_track_claim_kernel    a thread per QTK_CLAIM_PER_THREAD selected packets: a tracked packet that the state before the
 *                              call does not refuse enters the open-addressing table of selected positions (32-bit CAS into an
 *                              empty slot, atomicMin on a slot that holds its key: the lowest position of a key stays) and raises
 *                              its space's maximum: folded per lane, reduced per wave where the wave holds one space, then a
 *                              64-bit integer atomicMax
 *   quic_track_verdict_kernel  a thread per selected packet, behind the launch boundary: the verdict (a candidate is new if the
 *                              table holds its own position for its key), and a new packet's window bit ORed into its space's
 *                              scratch word when it lies within 64 of the space's next of after the call
 *   quic_track_apply_kernel    one thread per connection, launched twice around the scan levels of quic_parse_kernel.hip:
 *                              first the 0 / 1 flag "a space has a new packet"; then, with the flags scanned into positions, the
 *                              spaces moved on, their expected packet numbers stored, the scratch reset, and the connection
 *                              listed at its position.  No atomics decide a position: the list is ascending
 *
 * Maxima, minima and ORs of integers: whatever the order or the grouping, the outcome is the same.  No kernel has a private
 * segment or uses LDS.
 */
#include <hip/hip_runtime.h>

#include "internal.h"
#include "quic_scan.h"
#include "quic_track.h"

namespace ptls_hip {

constexpr int QTK_WG = 256;

namespace {

struct TrackOps {
    static __device__ __forceinline__ uint32_t cas(uint32_t *p, uint32_t expected, uint32_t desired)
    {
        return atomicCAS(p, expected, desired);
    }
    static __device__ __forceinline__ void min(uint32_t *p, uint32_t v)
    {
        atomicMin(p, v);
    }
};

/* a selected position's place in the state table (UINT64_MAX: not tracked), read from the call's inputs */
__device__ __forceinline__ uint64_t place_of(const QuicTrackArgs &a, uint64_t j)
{
    const uint32_t e = a.sel[j];
    if (e >= a.n)
        return UINT64_MAX;
    return quic_track_place(a.result[j], a.packed[j].key, a.count, a.info[e].type);
}

struct TrackKeys {
    const QuicTrackArgs &a;
    uint32_t m;
    /* (an occupant is a position some thread of this call entered: below m) */
    __device__ __forceinline__ bool same(uint32_t occ, uint64_t place, uint64_t pn) const
    {
        return occ < m && a.pn_out[occ] == pn && place_of(a, occ) == place;
    }
};

} // namespace

__global__ void __launch_bounds__(QTK_WG) quic_track_claim_kernel(const QuicTrackArgs a, const uint32_t m)
{
    /* A lane keeps the maximum for the space it last met and flushes it when the space changes; at the end a wave whose
     * lanes all hold one space (bulk traffic of one connection) reduces with shuffles and sends one atomic instead of 64. */
    constexpr uint64_t NOWHERE = UINT64_MAX;
    auto *acc = reinterpret_cast<unsigned long long *>(a.acc);
    const TrackKeys keys{a, m};
    uint64_t at = NOWHERE, top = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * QTK_WG + threadIdx.x; j < m; j += (uint64_t)gridDim.x * QTK_WG) {
        const uint64_t place = place_of(a, j);
        if (place == UINT64_MAX)
            continue;
        const ptls_hip_quic_pnspace_t st = a.spaces[place];
        const uint64_t pn = a.pn_out[j];
        if (quic_track_old(pn, st.next, st.window) != PTLS_HIP_QUIC_PN_NONE)
            continue;
        (void)quic_track_claim<TrackOps>(a.table, a.slots, (uint32_t)j, place, pn, keys);
        if (place != at) {
            if (at != NOWHERE)
                atomicMax(acc + 2 * at, (unsigned long long)top);
            at = place, top = pn + 1;
        } else {
            top = max(top, pn + 1);
        }
    }
    /* (every lane of the wave arrives here: the workgroup is whole waves and the loop has no early return) */
    const bool have = at != NOWHERE;
    const unsigned long long holders = __ballot(have);
    if (holders == 0)
        return;
    const uint64_t one = __shfl(at, __ffsll((long long)holders) - 1);
    if (__all(!have || at == one)) {
        uint64_t v = have ? top : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            v = max(v, (uint64_t)__shfl_xor(v, d));
        if ((threadIdx.x & 63) == 0)
            atomicMax(acc + 2 * one, (unsigned long long)v);
    } else if (have) {
        atomicMax(acc + 2 * at, (unsigned long long)top);
    }
}

__global__ void __launch_bounds__(QTK_WG) quic_track_verdict_kernel(const QuicTrackArgs a, const uint32_t m)
{
    auto *acc = reinterpret_cast<unsigned long long *>(a.acc);
    const TrackKeys keys{a, m};
    for (uint64_t j = (uint64_t)blockIdx.x * QTK_WG + threadIdx.x; j < m; j += (uint64_t)gridDim.x * QTK_WG) {
        uint32_t v = PTLS_HIP_QUIC_PN_NONE;
        const uint64_t place = place_of(a, j);
        if (place != UINT64_MAX) {
            const ptls_hip_quic_pnspace_t st = a.spaces[place];
            const uint64_t pn = a.pn_out[j];
            v = quic_track_old(pn, st.next, st.window);
            if (v == PTLS_HIP_QUIC_PN_NONE) {
                const uint32_t first = quic_track_find(a.table, a.slots, place, pn, keys);
                if (first == (uint32_t)j) {
                    v = PTLS_HIP_QUIC_PN_NEW;
                    const uint64_t bit = quic_track_bit(quic_track_next(st.next, a.acc[2 * place]), pn);
                    if (bit != 0)
                        atomicOr(acc + 2 * place + 1, (unsigned long long)bit);
                } else if (first != QTK_EMPTY) {
                    v = PTLS_HIP_QUIC_PN_DUPLICATE;
                }
            }
        }
        a.verdict[j] = v;
    }
}

__global__ void __launch_bounds__(QTK_WG) quic_track_apply_kernel(const QuicTrackArgs a, const int place)
{
    for (uint64_t c = (uint64_t)blockIdx.x * QTK_WG + threadIdx.x; c < a.count; c += (uint64_t)gridDim.x * QTK_WG) {
        const uint64_t top0 = a.acc[6 * c], top1 = a.acc[6 * c + 2], top2 = a.acc[6 * c + 4];
        const bool any = (top0 | top1 | top2) != 0;
        if (place == 0) {
            a.scan.l0[c] = any ? 1u : 0u;
            continue;
        }
        if (!any)
            continue;
#pragma unroll
        for (uint32_t s = 0; s < 3; ++s) {
            const uint64_t p = 3 * c + s, top = s == 0 ? top0 : s == 1 ? top1 : top2;
            if (top == 0)
                continue;
            ptls_hip_quic_pnspace_t st = a.spaces[p];
            quic_track_apply(&st, top, a.acc[2 * p + 1]);
            a.spaces[p] = st;
            if (a.expected_pn != nullptr && p < a.expected_count)
                a.expected_pn[p] = st.next;
            a.acc[2 * p] = 0;
            a.acc[2 * p + 1] = 0;
        }
        const uint32_t at = scan_at(a.scan, c); /* (the flag itself is gone: the scan wrote the prefix over it) */
        if (at < a.count)
            a.touched[at] = (uint32_t)c;
    }
}

int launch_quic_track_claim(const QuicTrackArgs &a, uint32_t m, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_track_claim_kernel, dim3(grid != 0 ? grid : 1), dim3(QTK_WG), 0, static_cast<hipStream_t>(stream), a, m);
    return (int)hipGetLastError();
}

int launch_quic_track_verdict(const QuicTrackArgs &a, uint32_t m, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_track_verdict_kernel, dim3(grid != 0 ? grid : 1), dim3(QTK_WG), 0, static_cast<hipStream_t>(stream), a, m);
    return (int)hipGetLastError();
}

int launch_quic_track_apply(const QuicTrackArgs &a, int place, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_track_apply_kernel, dim3(grid != 0 ? grid : 1), dim3(QTK_WG), 0, static_cast<hipStream_t>(stream), a, place);
    return (int)hipGetLastError();
}

} // namespace ptls_hip
