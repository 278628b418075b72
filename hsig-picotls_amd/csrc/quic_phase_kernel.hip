/*
 * quic_phase_kernel.hip -- QUIC receive keys chosen by Key Phase bit on the device, and key updates committed there
 * (include/ptls_hip.h 2j).  The rule is quic_phase.h's.
 *
 *   quic_unprotect_phase_kernel  quic_unprotect_kernel (the same body, quic_unprotect.h) plus one 16-byte load of the
 *                                connection's state, issued with the header's and the sample's loads; the record's key slot is
 *                                key + stride * (generation % 3), and the generation goes to gen_out
 *   quic_phase_mark_kernel       a thread per QPH_MARK_PER_THREAD selected packets: an authenticated packet of its connection's
 *                                current or next generation lowers one of the connection's two minima: folded per lane, reduced
 *                                per wave where the wave holds one place, then a 64-bit integer atomicMin (the outcome does
 *                                not depend on the order or the grouping)
 *   quic_phase_apply_kernel      one thread per connection, launched twice around the scan levels of quic_parse_kernel.hip:
 *                                first the 0 / 1 flag "has next-generation packets"; then, with the flags scanned into
 *                                positions, the entry moved on, the minima reset, and an updated connection listed at its
 *                                position.  No atomics decide a position: the list is ascending
 *
 * No kernel has a private segment; the two commit kernels use no LDS.
 */
#include <hip/hip_runtime.h>

#include "quic_scan.h"
#include "quic_unprotect.h"

namespace ptls_hip {

template <int ROUNDS>
__global__ void __launch_bounds__(QUIC_WG) quic_unprotect_phase_kernel(const QuicArgs a, const QuicPhaseArgs ph)
{
    quic_unprotect_packets<ROUNDS, true>(a, ph);
}

constexpr int QPH_WG = 256;

__global__ void __launch_bounds__(QPH_WG) quic_phase_mark_kernel(const QuicCommitArgs a, const uint32_t m)
{
    /* A lane keeps the minimum for the place it last met and flushes it when the place changes; at the end a wave whose
     * lanes all hold one place (bulk traffic of one connection) reduces with shuffles and sends one atomic instead of 64.
     * Minima of integers: whatever the grouping, the outcome is the same. */
    constexpr uint64_t NOWHERE = UINT64_MAX;
    auto *mins = reinterpret_cast<unsigned long long *>(a.mins);
    uint64_t at = NOWHERE, low = UINT64_MAX;
    for (uint64_t j = (uint64_t)blockIdx.x * QPH_WG + threadIdx.x; j < m; j += (uint64_t)gridDim.x * QPH_WG) {
        const uint32_t c = a.packed[j].key;
        if (c >= a.count)
            continue;
        const int cls = quic_phase_class(a.result[j], a.gen_out[j], a.phase[c].gen);
        if (cls == QPH_NONE)
            continue;
        const uint64_t place = 2 * (uint64_t)c + (cls == QPH_NEXT ? 0 : 1), pn = a.pn_out[j];
        if (place != at) {
            if (at != NOWHERE)
                atomicMin(mins + at, (unsigned long long)low);
            at = place, low = pn;
        } else {
            low = min(low, pn);
        }
    }
    /* (every lane of the wave arrives here: the workgroup is whole waves and the loop has no early return) */
    const bool have = at != NOWHERE;
    const unsigned long long holders = __ballot(have);
    if (holders == 0)
        return;
    const uint64_t one = __shfl(at, __ffsll((long long)holders) - 1);
    if (__all(!have || at == one)) {
        uint64_t v = have ? low : UINT64_MAX;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            v = min(v, (uint64_t)__shfl_xor(v, d));
        if ((threadIdx.x & 63) == 0)
            atomicMin(mins + one, (unsigned long long)v);
    } else if (have) {
        atomicMin(mins + at, (unsigned long long)low);
    }
}

__global__ void __launch_bounds__(QPH_WG) quic_phase_apply_kernel(const QuicCommitArgs a, const int place)
{
    for (uint64_t c = (uint64_t)blockIdx.x * QPH_WG + threadIdx.x; c < a.count; c += (uint64_t)gridDim.x * QPH_WG) {
        const uint64_t min_next = a.mins[2 * c], min_cur = a.mins[2 * c + 1];
        if (place == 0) {
            a.scan.l0[c] = quic_phase_updates(min_next) ? 1u : 0u;
            continue;
        }
        if (min_next == UINT64_MAX && min_cur == UINT64_MAX)
            continue;
        ptls_hip_quic_keyphase_t st = a.phase[c];
        quic_phase_apply(&st, min_next, min_cur);
        a.phase[c] = st;
        a.mins[2 * c] = UINT64_MAX;
        a.mins[2 * c + 1] = UINT64_MAX;
        if (quic_phase_updates(min_next)) { /* (the flag itself is gone: the scan wrote the prefix over it) */
            const uint32_t at = scan_at(a.scan, c);
            if (at < a.count)
                a.updated[at] = (uint32_t)c;
        }
    }
}

int launch_quic_unprotect_phase(int rounds, const QuicArgs &a, const QuicPhaseArgs &ph, unsigned grid, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (rounds == 10)
        hipLaunchKernelGGL(quic_unprotect_phase_kernel<10>, dim3(grid), dim3(QUIC_WG), 0, s, a, ph);
    else if (rounds == 14)
        hipLaunchKernelGGL(quic_unprotect_phase_kernel<14>, dim3(grid), dim3(QUIC_WG), 0, s, a, ph);
    else
        hipLaunchKernelGGL(quic_unprotect_phase_kernel<0>, dim3(grid), dim3(QUIC_WG), 0, s, a, ph);
    return (int)hipGetLastError();
}

int launch_quic_phase_mark(const QuicCommitArgs &a, uint32_t m, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_phase_mark_kernel, dim3(grid != 0 ? grid : 1), dim3(QPH_WG), 0, static_cast<hipStream_t>(stream), a, m);
    return (int)hipGetLastError();
}

int launch_quic_phase_apply(const QuicCommitArgs &a, int place, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_phase_apply_kernel, dim3(grid != 0 ? grid : 1), dim3(QPH_WG), 0, static_cast<hipStream_t>(stream), a, place);
    return (int)hipGetLastError();
}

} // namespace ptls_hip
