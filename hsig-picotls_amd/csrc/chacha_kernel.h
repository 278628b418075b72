/*
 * chacha_kernel.h -- what the two ChaCha20-Poly1305 record kernels share (chacha_kernel.hip: a lane owns whole 64-byte
 * blocks; chacha_runs_kernel.hip: the same arithmetic on data moved in contiguous runs): the lane combination, the key and
 * input loads, the header-protection mask, and what lane 0 does once the whole blocks are hashed (the last partial block, the
 * length block, the tag or its compare, then the header-protection step).  DESIGN.md §9.
 */
#pragma once

#include "batch_kernel.h"
#include "chacha20.h"
#include "poly1305.h"

namespace ptls_hip {

constexpr int CHACHA_WG = 256;

template <int B>
__device__ __forceinline__ uint32_t add_partner(uint32_t v)
{
    if constexpr (B == 0)
        return v + dpp_mov<DPP_QUAD_XOR1>(v);
    else if constexpr (B == 1)
        return v + dpp_mov<DPP_QUAD_XOR2>(v);
    else if constexpr (B == 2)
        return v + dpp_mov<DPP_ROW_HALF_MIRROR>(v);
    else if constexpr (B == 3)
        return v + dpp_mov<DPP_ROW_MIRROR>(v);
    else if constexpr (B == 4) {
        const auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false);
        return (uint32_t)p[0] + (uint32_t)p[1];
    } else {
        const auto p = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return (uint32_t)p[0] + (uint32_t)p[1];
    }
}

/* stage B of the lane combination (poly1305.h): called with every lane of the wave active.  The partner of stages 2 and
 * 3 is the mirrored lane of the other half, which holds that half's common sum after the stages before. */
template <int B, int LOG2G>
__device__ __forceinline__ void combine(Poly &acc, Poly &sq, uint32_t lane)
{
    if constexpr (B < LOG2G) {
        acc = poly_combine_stage(acc, sq, lane, B);
        acc = Poly{add_partner<B>(acc.h0), add_partner<B>(acc.h1), add_partner<B>(acc.h2), add_partner<B>(acc.h3),
                   add_partner<B>(acc.h4)};
        sq = poly_mul(sq, sq);
        combine<B + 1, LOG2G>(acc, sq, lane);
    }
}

/* 16 input bytes of which the first `avail` (any int; <= 0 none, >= 16 all) are read from p, with the TLS 1.3 content type
 * put at byte `tpos` when that is 0 .. 15 */
template <bool ALIGNED>
__device__ __forceinline__ V4 load_in(const uint8_t *p, int avail, int tpos, uint32_t ttype)
{
    V4 v;
    if (avail >= 16)
        v = load_full(p);
    else
        v = load_block<ALIGNED>(p, avail < 0 ? 0 : avail);
    if (tpos >= 0 && tpos < 16)
        v = put_byte(v, tpos, ttype);
    return v;
}

__device__ __forceinline__ ChaChaKey load_key(const ChaChaSlot *__restrict__ s)
{
    ChaChaKey k;
    k.k0 = s->key[0], k.k1 = s->key[1], k.k2 = s->key[2], k.k3 = s->key[3];
    k.k4 = s->key[4], k.k5 = s->key[5], k.k6 = s->key[6], k.k7 = s->key[7];
    k.n0 = k.n1 = k.n2 = 0;
    return k;
}

/* the header-protection mask of one sample: the first 16 keystream bytes of ChaCha20(hp key, counter = LE32(sample[0..4]),
 * nonce = sample[4..16]) (picotls's chacha20 cipher after do_init(sample), lib/cifra/chacha20.c:44-56) */
__device__ __forceinline__ V4 chacha_mask(const ChaChaSlot *__restrict__ slot, V4 sample)
{
    ChaChaKey k = load_key(slot);
    k.n0 = sample.w1, k.n1 = sample.w2, k.n2 = sample.w3;
    const ChaChaBlock b = chacha20_block(k, sample.w0);
    return V4{b.x0, b.x1, b.x2, b.x3};
}

/* one AAD's blocks, zero-padded to whole ones, on top of acc: the starting value of the place before the first chunk */
template <bool ALIGNED>
__device__ __forceinline__ Poly chacha_hash_aad(Poly acc, const uint8_t *aad_p, uint32_t A, Poly r1)
{
    const uint32_t na = A >> 4;
    for (uint32_t i = 0; i < na; ++i) {
        const V4 v = load_full(aad_p + (size_t)i * 16);
        acc = poly_step(acc, poly_block(v.w0, v.w1, v.w2, v.w3), r1);
    }
    if (A & 15u) {
        const V4 v = load_block<ALIGNED>(aad_p + (size_t)na * 16, (int)(A & 15u));
        acc = poly_step(acc, poly_block(v.w0, v.w1, v.w2, v.w3), r1);
    }
    return acc;
}

/* lane 0 of a record's group, with the sum over the AAD and every whole chunk in acc: the last, partial ChaCha block, the
 * length block, and the tag (seal: stored; open: compared, the result written) */
template <bool OPEN, bool ALIGNED>
__device__ __forceinline__ void chacha_tail_tag(const ChaChaArgs &a, uint64_t rec_i, const ChaChaKey &k, Poly acc, Poly r1,
                                                uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, const uint8_t *in_p,
                                                uint8_t *out_p, uint32_t L, uint32_t A, uint32_t in_len, bool tflag,
                                                uint32_t ttype)
{
    const uint32_t nfull = L >> 6;
    const uint32_t ntail = L & 63u;
    if (ntail != 0) {
        const size_t off = (size_t)nfull * 64;
        const ChaChaBlock ks = chacha20_block(k, nfull + 1);
        const int avail = (int)(in_len - nfull * 64u); /* input bytes of the tail: ntail, or ntail - 1 with the type */
        const int tpos = tflag ? (int)ntail - 1 : -1;
#define PTLS_HIP_CHACHA_TAIL(J, K0, K1, K2, K3)                                                                                    \
    if ((int)ntail > 16 * (J)) {                                                                                                   \
        const int nb = (int)ntail - 16 * (J) < 16 ? (int)ntail - 16 * (J) : 16;                                                    \
        const V4 iv = load_in<ALIGNED>(in_p + off + 16 * (J), avail - 16 * (J), tpos - 16 * (J), ttype);                            \
        const V4 ov = mask_block(V4{iv.w0 ^ ks.K0, iv.w1 ^ ks.K1, iv.w2 ^ ks.K2, iv.w3 ^ ks.K3}, nb);                               \
        const V4 cv = OPEN ? iv : ov;                                                                                              \
        acc = poly_step(acc, poly_block(cv.w0, cv.w1, cv.w2, cv.w3), r1);                                                          \
        store_block<ALIGNED>(out_p + off + 16 * (J), nb, ov);                                                                      \
    }
        PTLS_HIP_CHACHA_TAIL(0, x0, x1, x2, x3)
        PTLS_HIP_CHACHA_TAIL(1, x4, x5, x6, x7)
        PTLS_HIP_CHACHA_TAIL(2, x8, x9, x10, x11)
        PTLS_HIP_CHACHA_TAIL(3, x12, x13, x14, x15)
#undef PTLS_HIP_CHACHA_TAIL
    }
    /* LE64(aad_len) || LE64(len), then the tag */
    acc = poly_step(acc, poly_block(A, 0, L, 0), r1);
    uint32_t t0, t1, t2, t3;
    poly_finish(acc, s0, s1, s2, s3, t0, t1, t2, t3);
    if (OPEN) {
        const V4 rt = load_full(in_p + L);
        const bool ok = ((rt.w0 ^ t0) | (rt.w1 ^ t1) | (rt.w2 ^ t2) | (rt.w3 ^ t3)) == 0;
        a.result[rec_i] = ok ? (uint64_t)L : ~(uint64_t)0;
    } else {
        store_full(out_p + L, V4{t0, t1, t2, t3});
    }
}

/* header protection, after the record (seal with supp descriptors; called by every lane): the sample may cover the tag,
 * and other lanes of this wave wrote most of it (the release / acquire pair completes their stores before the read, as in
 * the AES batch kernel) */
__device__ __forceinline__ void chacha_hp_step(const ChaChaArgs &a, uint64_t rec_i, bool lane0)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (lane0) {
        const ptls_hip_supp_t sp = a.supp[rec_i];
        if ((sp.flags & PTLS_HIP_SUPP_ENABLE) && sp.hp_key < a.hp_nslots)
            store_full(a.mask + sp.mask_off, chacha_mask(a.hp_slots + sp.hp_key, load_full(a.out + sp.sample_off)));
    }
}

} // namespace ptls_hip
