/*
 * quic_unprotect.h -- the body of the receive-side header kernels (device only): quic_kernel.hip's quic_unprotect_kernel and
 * quic_phase_kernel.hip's quic_unprotect_phase_kernel are this one function, without and with the choice of the key by Key
 * Phase bit (quic_phase.h).  The header arithmetic is quic.h's.
 */
#pragma once

#include "batch_kernel.h"
#include "chacha20.h"
#include "quic.h"
#include "quic_phase.h"

namespace ptls_hip {

constexpr int QUIC_WG = 256;

/* ROUNDS 10 / 14: AES-128 / AES-256 header protection; 0: ChaCha20 (no LDS).  PHASE: the record's key slot is chosen from
 * ph.phase[p.key] and the unmasked Key Phase bit, and the generation goes to ph.gen_out[i]; the 16-byte state is loaded with
 * the header's and the sample's bytes, before the mask is known.  p.key is inside ph.phase by the select rule of the caller. */
template <int ROUNDS, bool PHASE>
__device__ __forceinline__ void quic_unprotect_packets(const QuicArgs &a, const QuicPhaseArgs &ph)
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
        [[maybe_unused]] ptls_hip_quic_keyphase_t st{};
        if constexpr (PHASE)
            st = ph.phase[p.key]; /* ... and so is the connection's state */
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
        if constexpr (PHASE) {
            const uint32_t g = quic_phase_gen(quic_phase_first_byte(h.first, masked, m0), pn, st.gen, st.first_pn);
            r.key = quic_phase_slot(p.key, ph.stride, g);
            ph.gen_out[i] = g;
        }
        r.flags = 0;
        a.recs[i] = r;
        if (a.recs_ord != nullptr)
            a.recs_ord[t] = r;
    }
}

} // namespace ptls_hip
