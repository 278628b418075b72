/* quic_scan.h -- device only: what the QUIC kernels share around the scan levels of quic_parse_kernel.hip (internal.h ScanRef) */
#pragma once

#include "internal.h"

namespace ptls_hip {

/* the exclusive prefix of position j over scanned levels (s by value: three pointers; taken by reference, the compact
 * kernel of quic_rx_kernel.hip came out one instruction longer than with the lookup written out) */
__device__ __forceinline__ uint32_t scan_at(const ScanRef s, uint64_t j)
{
    uint32_t at = s.l0[j];
    if (s.l1 != nullptr)
        at += s.l1[j / QP_SCAN_SPAN];
    if (s.l2 != nullptr)
        at += s.l2[j / ((uint64_t)QP_SCAN_SPAN * QP_SCAN_SPAN)];
    return at;
}

/* the sum over the wave's 64 lanes, in every lane (integers: the order of addition does not matter) */
__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v += __shfl_xor(v, d);
    return v;
}

} // namespace ptls_hip
