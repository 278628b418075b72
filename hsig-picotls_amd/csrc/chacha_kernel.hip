/*
 * chacha_kernel.hip -- ChaCha20-Poly1305 (RFC 8439 §2.8; picotls lib/chacha20poly1305.h:77-150) for the records of a batch,
 * and ChaCha20 header-protection masks (RFC 9001 §5.4.4).  DESIGN.md §9.
 *
 * G lanes (1, 4, 16 or 64) share one record.  Every lane computes the record's ChaCha block 0 (the one-time Poly1305 key
 * r, s) and the powers r^2, r^3, r^4 and r^(4G) in its own registers: r belongs to the record, so there is nothing to
 * look up, and on a SIMD the lanes of a group compute it in the time one lane would.  The whole 64-byte ChaCha blocks are
 * dealt to the lanes from the end of the data (poly1305.h describes the split); a lane encrypts its block, hashes the four
 * ciphertext blocks against r^4 .. r on top of acc r^(4G), and writes it.  The lanes' sums are joined by log2 G stages of one
 * multiplication and one DPP / permlane exchange each; lane 0 then runs the last partial ChaCha block, the length block
 * and the tag.  No LDS, no scratch: all state is in named registers (chacha20.h, poly1305.h).  What this kernel shares with
 * chacha_runs_kernel.hip (the same arithmetic on data moved in contiguous runs, for host memory) is in chacha_kernel.h.
 *
 * Exact bytes: whole blocks are single 16-byte accesses inside the record; partial blocks go through load_block /
 * store_block of batch_kernel.h (whole dwords inside the record, then a 16-bit and / or an 8-bit access; byte by byte when
 * the layout is not 16-byte aligned).  Nothing outside a record's input (+ tag on open), AAD and output is touched.
 */
#include "chacha_kernel.h"

namespace ptls_hip {

template <int G, bool OPEN, bool ALIGNED>
__global__ void __launch_bounds__(CHACHA_WG) chacha20poly1305_batch_kernel(const ChaChaArgs a)
{
    static_assert(G == 1 || G == 4 || G == 16 || G == 64, "lanes per record");
    constexpr int LOG2G = G == 1 ? 0 : G == 4 ? 2 : G == 16 ? 4 : 6;
    const uint64_t gid = (uint64_t)blockIdx.x * CHACHA_WG + threadIdx.x;
    const uint64_t rec_i = gid / G;
    const uint32_t l = (uint32_t)(gid % G);
    const bool valid = rec_i < a.n;

    ptls_hip_record_t rec = a.one;
    if (a.recs != nullptr && valid)
        rec = a.recs[rec_i];
    const uint32_t L = valid ? rec.len : 0u, A = valid ? rec.aad_len : 0u;
    const bool tflag = !OPEN && (rec.flags & 1u) != 0 && L > 0;
    const uint32_t ttype = (rec.flags >> 8) & 0xffu;
    const uint32_t in_len = tflag ? L - 1 : L; /* bytes read from the input; byte L - 1 is the content type otherwise */
    const uint8_t *in_p = a.in + rec.in_off;
    const uint8_t *aad_p = a.aad + rec.aad_off;
    uint8_t *out_p = a.out + rec.out_off;

    /* the record's one-time key and the powers of r */
    const ChaChaSlot *slot = a.slots + (valid ? rec.key : 0u);
    ChaChaKey k = load_key(slot);
    chacha_nonce(k, slot->iv[0], slot->iv[1], slot->iv[2], rec.seq);
    Poly r1, r2, r3, r4, rG;
    uint32_t s0, s1, s2, s3;
    {
        const ChaChaBlock b0 = chacha20_block(k, 0);
        r1 = poly_clamp_r(b0.x0, b0.x1, b0.x2, b0.x3);
        s0 = b0.x4, s1 = b0.x5, s2 = b0.x6, s3 = b0.x7;
    }
    r2 = poly_mul(r1, r1);
    r3 = poly_mul(r2, r1);
    r4 = poly_mul(r2, r2);
    rG = r4;
#pragma unroll
    for (int b = 0; b < LOG2G; ++b)
        rG = poly_mul(rG, rG);

    /* whole ChaCha blocks, dealt from the end: place q = chunk + pad, lane q % G, trip q / G */
    const uint32_t nfull = L >> 6;
    const uint32_t T = valid ? nfull / G + 1 : 0u;
    const uint32_t pad = T * G - nfull; /* 1 .. G */

    Poly acc = poly_zero();
    if (valid && l == pad - 1) { /* the place before the first chunk: the AAD, zero-padded to whole blocks */
        acc = chacha_hash_aad<ALIGNED>(acc, aad_p, A, r1);
    }

    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t q = t * G + l;
        if (q < pad)
            continue; /* trip 0 only: an empty place (or the AAD's) */
        const uint32_t c = q - pad;
        const size_t off = (size_t)c * 64;
        const ChaChaBlock ks = chacha20_block(k, c + 1);
        V4 i0, i1, i2, i3;
        i0 = load_full(in_p + off);
        i1 = load_full(in_p + off + 16);
        i2 = load_full(in_p + off + 32);
        if (off + 64 <= in_len)
            i3 = load_full(in_p + off + 48);
        else /* the record ends with this block and its last byte is the content type */
            i3 = load_in<ALIGNED>(in_p + off + 48, 15, 15, ttype);
        const V4 o0 = V4{i0.w0 ^ ks.x0, i0.w1 ^ ks.x1, i0.w2 ^ ks.x2, i0.w3 ^ ks.x3};
        const V4 o1 = V4{i1.w0 ^ ks.x4, i1.w1 ^ ks.x5, i1.w2 ^ ks.x6, i1.w3 ^ ks.x7};
        const V4 o2 = V4{i2.w0 ^ ks.x8, i2.w1 ^ ks.x9, i2.w2 ^ ks.x10, i2.w3 ^ ks.x11};
        const V4 o3 = V4{i3.w0 ^ ks.x12, i3.w1 ^ ks.x13, i3.w2 ^ ks.x14, i3.w3 ^ ks.x15};
        const V4 c0 = OPEN ? i0 : o0, c1 = OPEN ? i1 : o1, c2 = OPEN ? i2 : o2, c3 = OPEN ? i3 : o3;
        acc = poly_chunk(acc, rG, poly_block(c0.w0, c0.w1, c0.w2, c0.w3), poly_block(c1.w0, c1.w1, c1.w2, c1.w3),
                         poly_block(c2.w0, c2.w1, c2.w2, c2.w3), poly_block(c3.w0, c3.w1, c3.w2, c3.w3), r1, r2, r3, r4);
        store_full(out_p + off, o0);
        store_full(out_p + off + 16, o1);
        store_full(out_p + off + 32, o2);
        store_full(out_p + off + 48, o3);
    }

    /* every lane of the wave is here again, whatever its group's trip count was */
    {
        Poly sq = r4;
        combine<0, LOG2G>(acc, sq, l);
    }

    if (valid && l == 0)
        chacha_tail_tag<OPEN, ALIGNED>(a, rec_i, k, acc, r1, s0, s1, s2, s3, in_p, out_p, L, A, in_len, tflag, ttype);

    if (!OPEN && a.supp != nullptr)
        chacha_hp_step(a, rec_i, valid && l == 0);
}

/* standalone masks (the receive side): one thread per descriptor */
__global__ void __launch_bounds__(256) chacha20_mask_kernel(const ptls_hip_supp_t *__restrict__ supp, uint32_t n,
                                                            const uint8_t *__restrict__ src, uint8_t *__restrict__ mask,
                                                            const ChaChaSlot *__restrict__ hp_slots, uint32_t hp_nslots)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const ptls_hip_supp_t sp = supp[i];
        if ((sp.flags & PTLS_HIP_SUPP_ENABLE) && sp.hp_key < hp_nslots)
            store_full(mask + sp.mask_off, chacha_mask(hp_slots + sp.hp_key, load_full(src + sp.sample_off)));
    }
}

/* key slots from raw keys and IVs: one thread per slot */
__global__ void __launch_bounds__(256) chacha_keysetup_kernel(ChaChaSlot *__restrict__ slots, const uint8_t *__restrict__ keys,
                                                              const uint8_t *__restrict__ ivs, uint32_t first, uint32_t count)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count)
        return;
    ChaChaSlot s;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const uint8_t *p = keys + (size_t)i * 32 + 4 * w;
        s.key[w] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    }
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        const uint8_t *p = ivs + (size_t)i * 12 + 4 * w;
        s.iv[w] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    }
    slots[first + i] = s;
}

template <int G, bool OPEN>
static hipError_t launch_chacha_g(unsigned grid, hipStream_t s, const ChaChaArgs &a, bool aligned)
{
    if (aligned)
        hipLaunchKernelGGL((chacha20poly1305_batch_kernel<G, OPEN, true>), dim3(grid), dim3(CHACHA_WG), 0, s, a);
    else
        hipLaunchKernelGGL((chacha20poly1305_batch_kernel<G, OPEN, false>), dim3(grid), dim3(CHACHA_WG), 0, s, a);
    return hipGetLastError();
}

int launch_chacha_batch(int lanes, bool open, void *stream, const ChaChaArgs &a, bool aligned)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t threads = (uint64_t)a.n * (uint64_t)lanes;
    const unsigned grid = (unsigned)((threads + CHACHA_WG - 1) / CHACHA_WG);
    switch (lanes) {
    case 1:
        return (int)(open ? launch_chacha_g<1, true>(grid, s, a, aligned) : launch_chacha_g<1, false>(grid, s, a, aligned));
    case 4:
        return (int)(open ? launch_chacha_g<4, true>(grid, s, a, aligned) : launch_chacha_g<4, false>(grid, s, a, aligned));
    case 16:
        return (int)(open ? launch_chacha_g<16, true>(grid, s, a, aligned) : launch_chacha_g<16, false>(grid, s, a, aligned));
    case 64:
        return (int)(open ? launch_chacha_g<64, true>(grid, s, a, aligned) : launch_chacha_g<64, false>(grid, s, a, aligned));
    }
    return (int)hipErrorInvalidValue;
}

int launch_chacha_mask(const ptls_hip_supp_t *supp, uint32_t n, const uint8_t *src, uint8_t *mask, const ChaChaSlot *hp_slots,
                       uint32_t hp_nslots, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(chacha20_mask_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), supp, n, src, mask,
                       hp_slots, hp_nslots);
    return (int)hipGetLastError();
}

int launch_chacha_keysetup(ChaChaSlot *slots, const uint8_t *keys, const uint8_t *ivs, uint32_t first, uint32_t count,
                           void *stream)
{
    hipLaunchKernelGGL(chacha_keysetup_kernel, dim3((count + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), slots,
                       keys, ivs, first, count);
    return (int)hipGetLastError();
}

} // namespace ptls_hip
