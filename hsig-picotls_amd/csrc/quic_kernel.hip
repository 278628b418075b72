/*
 * quic_kernel.hip -- QUIC header protection on the device, around the record kernels.
 *
 * quic_unprotect_kernel runs before an open launch: one thread per plan position takes the packet's header-protection mask
 * from its sample (AES-ECB with the LDS T-tables of aesecb_batch_kernel, or the first ChaCha20 keystream bytes), removes it
 * from the first byte and the packet-number bytes in place, decodes the full packet number (RFC 9000 A.3) and writes the
 * record descriptor the open kernel then reads: the packet-number length, and with it the AAD length, the input offset, the
 * record length and the nonce, are known only here.  quic_protect_kernel runs after a seal launch with header-protection
 * masks (seal_batch_supp) and applies mask i to the header of packet i.  The header arithmetic is quic.h's.
 *
 * Exact bytes: the sample is one 16-byte load inside the packet (the host refuses packets shorter than pn_offset + 20),
 * header bytes are single-byte loads and stores, and nothing but the first byte and the packet-number bytes is written.
 */
#include "quic_unprotect.h"

namespace ptls_hip {

/* ROUNDS 10 / 14: AES-128 / AES-256 header protection; 0: ChaCha20 (no LDS).  The body is quic_unprotect.h's, shared with
 * quic_phase_kernel.hip */
template <int ROUNDS>
__global__ void __launch_bounds__(QUIC_WG) quic_unprotect_kernel(const QuicArgs a)
{
    quic_unprotect_packets<ROUNDS, false>(a, QuicPhaseArgs{});
}

/* after seal_batch_supp on the same stream: mask i sits at mask + 16 i */
__global__ void __launch_bounds__(QUIC_WG) quic_protect_kernel(const ptls_hip_quic_packet_t *__restrict__ pkts, uint32_t n,
                                                               uint8_t *pkt, const uint8_t *__restrict__ mask)
{
    for (uint32_t i = blockIdx.x * QUIC_WG + threadIdx.x; i < n; i += gridDim.x * QUIC_WG) {
        const ptls_hip_quic_packet_t p = pkts[i];
        const uint32_t *m = reinterpret_cast<const uint32_t *>(mask + 16 * (size_t)i);
        quic_protect_header(pkt + p.pkt_off, p.pn_offset, p.pn_len, m[0], m[1]);
    }
}

int launch_quic_unprotect(int rounds, const QuicArgs &a, unsigned grid, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (rounds == 10)
        hipLaunchKernelGGL(quic_unprotect_kernel<10>, dim3(grid), dim3(QUIC_WG), 0, s, a);
    else if (rounds == 14)
        hipLaunchKernelGGL(quic_unprotect_kernel<14>, dim3(grid), dim3(QUIC_WG), 0, s, a);
    else
        hipLaunchKernelGGL(quic_unprotect_kernel<0>, dim3(grid), dim3(QUIC_WG), 0, s, a);
    return (int)hipGetLastError();
}

int launch_quic_protect(const ptls_hip_quic_packet_t *pkts, uint32_t n, uint8_t *pkt, const uint8_t *mask, unsigned grid,
                        void *stream)
{
    hipLaunchKernelGGL(quic_protect_kernel, dim3(grid), dim3(QUIC_WG), 0, static_cast<hipStream_t>(stream), pkts, n, pkt, mask);
    return (int)hipGetLastError();
}

} // namespace ptls_hip
