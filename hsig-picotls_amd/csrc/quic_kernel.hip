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
#include "batch_kernel.h"
#include "chacha20.h"
#include "quic.h"

namespace ptls_hip {

constexpr int QUIC_WG = 256;

/* ROUNDS 10 / 14: AES-128 / AES-256 header protection; 0: ChaCha20 (no LDS) */
template <int ROUNDS>
__global__ void __launch_bounds__(QUIC_WG) quic_unprotect_kernel(const QuicArgs a)
{
    constexpr bool AES = ROUNDS != 0;
    __shared__ __attribute__((aligned(16))) uint8_t lds[AES ? LDS_AES + 65536 : 16];
    if (AES) {
        build_aes_tables<QUIC_WG>(lds, LDS_AES, a.t0);
        __syncthreads();
    }
    [[maybe_unused]] const uint32_t lb_aes = (uint32_t)(threadIdx.x & 31) * 4u | LDS_AES;
    for (uint32_t t = blockIdx.x * QUIC_WG + threadIdx.x; t < a.n; t += gridDim.x * QUIC_WG) {
        const uint32_t i = a.order != nullptr ? a.order[t] : t;
        const ptls_hip_quic_packet_t p = a.pkts[i];
        uint8_t *hdr = a.pkt + p.pkt_off;
        const bool masked = (p.flags & PTLS_HIP_QUIC_UNPROTECTED) == 0;
        const QuicHeaderBytes h = quic_load_header(hdr, p.pn_offset); /* issued with the sample's load */
        uint32_t m0 = 0, m1 = 0;
        if (masked) {
            const V4 sample = load_full(hdr + p.pn_offset + 4);
            if constexpr (AES) {
                const V4 m = aes_encrypt<ROUNDS>(lds, lb_aes, a.hp_slots[p.hp_key].rk, sample);
                m0 = m.w0, m1 = m.w1;
            } else {
                /* picotls's chacha20 cipher after do_init(sample): counter = LE32(sample[0..4]), nonce = sample[4..16] */
                const ChaChaSlot *__restrict__ s = a.hp_chacha + p.hp_key;
                ChaChaKey k;
                k.k0 = s->key[0], k.k1 = s->key[1], k.k2 = s->key[2], k.k3 = s->key[3];
                k.k4 = s->key[4], k.k5 = s->key[5], k.k6 = s->key[6], k.k7 = s->key[7];
                k.n0 = sample.w1, k.n1 = sample.w2, k.n2 = sample.w3;
                const ChaChaBlock b = chacha20_block(k, sample.w0);
                m0 = b.x0, m1 = b.x1;
            }
        }
        uint64_t truncated;
        const uint32_t pn_len = quic_unprotect_header(hdr, p.pn_offset, h, masked, m0, m1, &truncated);
        const uint64_t pn = quic_decode_pn(p.pn, truncated, pn_len);
        a.pn_out[i] = pn;

        ptls_hip_record_t r;
        r.aad_off = p.pkt_off;
        r.aad_len = (uint32_t)p.pn_offset + pn_len;
        r.in_off = p.pkt_off + r.aad_len;
        r.len = p.pkt_len - r.aad_len - 16u; /* >= 0: pkt_len >= pn_offset + 20 */
        r.out_off = p.data_off;
        r.seq = pn;
        r.key = p.key;
        r.flags = 0;
        a.recs[i] = r;
        if (a.recs_ord != nullptr)
            a.recs_ord[t] = r;
    }
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
