/*
 * quic_slice_kernel.hip -- the header return of the copy transport's QUIC open slices (pipeline.cpp).
 *
 * quic_unprotect_kernel has unprotected the headers of the slice's packets in the slot's input staging.  The caller's h_pkt
 * must receive exactly those 1 + pn_len bytes per packet, and pn_len is known only on the device.  Copying the packets back
 * would cost the input's bandwidth a second time, so quic_pack_headers_kernel runs behind quic_unprotect_kernel on the
 * slice's stream and packs, for slice packet t, 8 bytes at packed + 8 t:
 *     byte 0     the number of header bytes to place: 0 with PTLS_HIP_QUIC_UNPROTECTED (nothing was unprotected), else
 *                1 + pn_len
 *     byte 1     the first byte
 *     byte 2..5  the packet-number bytes (those past pn_len are 0)
 *     byte 6..7  0
 * One copy per slice brings the entries to pinned slot memory and the host places them (slot_wait).
 *
 * One thread per packet.  The header bytes are the five single-byte loads of quic_load_header (quic.h), inside the packet
 * because the sample starts at pn_offset + 4; they are selected under compile-time indices, so there is no scratch, and no
 * LDS.  The entry leaves as one 8-byte store.
 */
#include <hip/hip_runtime.h>

#include "internal.h"
#include "quic.h"

namespace ptls_hip {

constexpr int QUIC_SLICE_WG = 256;

__global__ void __launch_bounds__(QUIC_SLICE_WG) quic_pack_headers_kernel(const ptls_hip_quic_packet_t *__restrict__ pkts, uint32_t n,
                                                                         const uint8_t *__restrict__ pkt, uint2 *__restrict__ packed)
{
    for (uint32_t t = blockIdx.x * QUIC_SLICE_WG + threadIdx.x; t < n; t += gridDim.x * QUIC_SLICE_WG) {
        const ptls_hip_quic_packet_t p = pkts[t];
        const QuicHeaderBytes h = quic_load_header(pkt + p.pkt_off, p.pn_offset);
        /* the header is unprotected: quic_unprotect_header without a mask reads pn_len and writes nothing */
        uint64_t truncated;
        const uint32_t pn_len = quic_unprotect_header(nullptr, p.pn_offset, h, false, 0, 0, &truncated);
        const uint32_t count = (p.flags & PTLS_HIP_QUIC_UNPROTECTED) != 0 ? 0u : 1u + pn_len;
        uint2 e;
        e.x = count | h.first << 8 | h.b0 << 16 | (pn_len > 1 ? h.b1 << 24 : 0u);
        e.y = (pn_len > 2 ? h.b2 : 0u) | (pn_len > 3 ? h.b3 << 8 : 0u);
        packed[t] = e;
    }
}

int launch_quic_pack_headers(const ptls_hip_quic_packet_t *pkts, uint32_t n, const uint8_t *pkt, void *packed, void *stream)
{
    if (n == 0)
        return 0;
    hipLaunchKernelGGL(quic_pack_headers_kernel, dim3((n + QUIC_SLICE_WG - 1) / QUIC_SLICE_WG), dim3(QUIC_SLICE_WG), 0,
                       static_cast<hipStream_t>(stream), pkts, n, pkt, static_cast<uint2 *>(packed));
    return (int)hipGetLastError();
}

} // namespace ptls_hip
