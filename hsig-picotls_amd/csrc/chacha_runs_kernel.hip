/*
 * chacha_runs_kernel.hip -- ChaCha20-Poly1305 for records that the kernel reads from and writes to pinned HOST memory over
 * PCIe (the pipelines' mapped transport, pipeline.cpp).  The arithmetic, the deal of the blocks from the end of the data,
 * the AAD's place, the lane combination, lane 0's tail and tag and the header-protection step are those of
 * chacha_kernel.hip (chacha_kernel.h, chacha20.h, poly1305.h).  What differs is how a trip's 64 G bytes reach the G lanes of
 * a record.  There a lane loads its own 64-byte block as four 16-byte accesses, so one wave instruction touches 16 bytes of
 * every 64: fine from HBM behind the caches, but over the link the run length per instruction decides the rate
 * (mapped_lanes in pipeline.cpp).  Here instruction j has lane l move the 16-byte piece j G + l of the trip: one contiguous
 * run of 16 G bytes per group and instruction (1 KiB at G = 64), and a 4 x 4 transpose inside each quad (two DPP quad_perm
 * stages) then gives every lane the four pieces of one block.  chacha_runs.h holds the piece map and the transpose's rule;
 * the stores run the transpose again and write the same runs.  DESIGN.md §9.
 *
 * Nothing between the loads and the stores of a trip may be skipped by a lane, because the quad's other lanes need its
 * pieces: a lane without a block in trip 0 predicates its loads, its block and its stores instead of leaving the trip.  The
 * groups of one wave may still run different trip counts; a group is at least a quad, so the exchange stays inside lanes
 * that are active together.  No LDS, no scratch.
 *
 * Exact bytes: a piece before the record's first byte is never loaded or stored, no piece ends past the whole blocks, and
 * with the TLS 1.3 content type in byte L - 1 of a record of whole blocks the last piece goes through load_in, which does
 * not read that byte.  The tail, the tag and the AAD go through the helpers of chacha_kernel.h.
 */
#include "chacha_kernel.h"
#include "chacha_runs.h"

namespace ptls_hip {

/* stage B of the quad transpose on one word of the register pair (lo, hi) */
template <int B>
__device__ __forceinline__ void runs_trade(uint32_t &lo, uint32_t &hi, uint32_t l)
{
    const uint32_t give = runs_send(lo, hi, l, B);
    runs_recv(lo, hi, l, B, B == 0 ? dpp_mov<DPP_QUAD_XOR1>(give) : dpp_mov<DPP_QUAD_XOR2>(give));
}

template <int B>
__device__ __forceinline__ void runs_trade(V4 &lo, V4 &hi, uint32_t l)
{
    runs_trade<B>(lo.w0, hi.w0, l);
    runs_trade<B>(lo.w1, hi.w1, l);
    runs_trade<B>(lo.w2, hi.w2, l);
    runs_trade<B>(lo.w3, hi.w3, l);
}

/* [lane a of the quad][register j] -> [lane j][register a]; every lane of the quad active */
__device__ __forceinline__ void runs_transpose(V4 &v0, V4 &v1, V4 &v2, V4 &v3, uint32_t l)
{
    runs_trade<0>(v0, v1, l);
    runs_trade<0>(v2, v3, l);
    runs_trade<1>(v0, v2, l);
    runs_trade<1>(v1, v3, l);
}

/* lane l of the wave's G-lane group takes v from lane src of the group (every lane of the wave active) */
template <int G>
__device__ __forceinline__ uint32_t runs_fetch(uint32_t v, uint32_t src)
{
    const uint32_t wl = threadIdx.x & 63u;
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)((((wl & ~(uint32_t)(G - 1)) | src) << 2)), (int)v);
}

template <int G, bool OPEN, bool ALIGNED>
__global__ void __launch_bounds__(CHACHA_WG) chacha20poly1305_runs_kernel(const ChaChaArgs a)
{
    static_assert(G == 4 || G == 16 || G == 64, "lanes per record");
    constexpr int LOG2G = G == 4 ? 2 : G == 16 ? 4 : 6;
    const uint64_t gid = (uint64_t)blockIdx.x * CHACHA_WG + threadIdx.x;
    const uint64_t rec_i = gid / G;
    const uint32_t l = (uint32_t)(gid % G);
    const uint32_t lam = runs_lambda(G, l);
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

    /* whole ChaCha blocks, dealt from the end: place q = chunk + pad, in trip q / G the block of the lane with lambda = q % G */
    const uint32_t nfull = L >> 6;
    const uint32_t T = valid ? runs_trips(G, nfull) : 0u;
    const uint32_t pad = T * G - nfull; /* 1 .. G */

    Poly acc = poly_zero();
    if (valid && lam == pad - 1) /* the place before the first chunk: the AAD, zero-padded to whole blocks */
        acc = chacha_hash_aad<ALIGNED>(acc, aad_p, A, r1);

    for (uint32_t t = 0; t < T; ++t) {
        /* this lane's four pieces of the trip's runs; only trip 0 has pieces before the data */
        const int64_t p0 = runs_piece_off(G, nfull, t, 0, l), p1 = runs_piece_off(G, nfull, t, 1, l);
        const int64_t p2 = runs_piece_off(G, nfull, t, 2, l), p3 = runs_piece_off(G, nfull, t, 3, l);
        V4 v0{0, 0, 0, 0}, v1 = v0, v2 = v0, v3 = v0;
        if (p0 >= 0)
            v0 = load_full(in_p + p0);
        if (p1 >= 0)
            v1 = load_full(in_p + p1);
        if (p2 >= 0)
            v2 = load_full(in_p + p2);
        if (p3 >= 0) { /* the trip's last piece may be the record's last, and its last byte the content type */
            if ((uint64_t)p3 + 16 <= in_len)
                v3 = load_full(in_p + p3);
            else
                v3 = load_in<ALIGNED>(in_p + p3, 15, 15, ttype);
        }
        runs_transpose(v0, v1, v2, v3, l);
        if (t * G + lam >= pad) { /* v0 .. v3: the block at place lambda of this trip */
            const ChaChaBlock ks = chacha20_block(k, t * G + lam - pad + 1);
            const V4 i0 = v0, i1 = v1, i2 = v2, i3 = v3;
            v0 = V4{i0.w0 ^ ks.x0, i0.w1 ^ ks.x1, i0.w2 ^ ks.x2, i0.w3 ^ ks.x3};
            v1 = V4{i1.w0 ^ ks.x4, i1.w1 ^ ks.x5, i1.w2 ^ ks.x6, i1.w3 ^ ks.x7};
            v2 = V4{i2.w0 ^ ks.x8, i2.w1 ^ ks.x9, i2.w2 ^ ks.x10, i2.w3 ^ ks.x11};
            v3 = V4{i3.w0 ^ ks.x12, i3.w1 ^ ks.x13, i3.w2 ^ ks.x14, i3.w3 ^ ks.x15};
            const V4 c0 = OPEN ? i0 : v0, c1 = OPEN ? i1 : v1, c2 = OPEN ? i2 : v2, c3 = OPEN ? i3 : v3;
            acc = poly_chunk(acc, rG, poly_block(c0.w0, c0.w1, c0.w2, c0.w3), poly_block(c1.w0, c1.w1, c1.w2, c1.w3),
                             poly_block(c2.w0, c2.w1, c2.w2, c2.w3), poly_block(c3.w0, c3.w1, c3.w2, c3.w3), r1, r2, r3, r4);
        }
        runs_transpose(v0, v1, v2, v3, l);
        if (p0 >= 0)
            store_full(out_p + p0, v0);
        if (p1 >= 0)
            store_full(out_p + p1, v1);
        if (p2 >= 0)
            store_full(out_p + p2, v2);
        if (p3 >= 0)
            store_full(out_p + p3, v3);
    }

    /* every lane of the wave is here again, whatever its group's trip count was: the sum of place m goes to lane m, where
     * the combination expects it (G = 4: lambda is the identity) */
    if constexpr (G > 4) {
        const uint32_t src = runs_acc_source(G, l);
        acc = Poly{runs_fetch<G>(acc.h0, src), runs_fetch<G>(acc.h1, src), runs_fetch<G>(acc.h2, src), runs_fetch<G>(acc.h3, src),
                   runs_fetch<G>(acc.h4, src)};
    }
    {
        Poly sq = r4;
        combine<0, LOG2G>(acc, sq, l);
    }

    if (valid && l == 0)
        chacha_tail_tag<OPEN, ALIGNED>(a, rec_i, k, acc, r1, s0, s1, s2, s3, in_p, out_p, L, A, in_len, tflag, ttype);

    if (!OPEN && a.supp != nullptr)
        chacha_hp_step(a, rec_i, valid && l == 0);
}

template <int G, bool OPEN>
static hipError_t launch_runs_g(unsigned grid, hipStream_t s, const ChaChaArgs &a, bool aligned)
{
    if (aligned)
        hipLaunchKernelGGL((chacha20poly1305_runs_kernel<G, OPEN, true>), dim3(grid), dim3(CHACHA_WG), 0, s, a);
    else
        hipLaunchKernelGGL((chacha20poly1305_runs_kernel<G, OPEN, false>), dim3(grid), dim3(CHACHA_WG), 0, s, a);
    return hipGetLastError();
}

int launch_chacha_runs(int lanes, bool open, void *stream, const ChaChaArgs &a, bool aligned)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t threads = (uint64_t)a.n * (uint64_t)lanes;
    const unsigned grid = (unsigned)((threads + CHACHA_WG - 1) / CHACHA_WG);
    switch (lanes) {
    case 4:
        return (int)(open ? launch_runs_g<4, true>(grid, s, a, aligned) : launch_runs_g<4, false>(grid, s, a, aligned));
    case 16:
        return (int)(open ? launch_runs_g<16, true>(grid, s, a, aligned) : launch_runs_g<16, false>(grid, s, a, aligned));
    case 64:
        return (int)(open ? launch_runs_g<64, true>(grid, s, a, aligned) : launch_runs_g<64, false>(grid, s, a, aligned));
    }
    return (int)hipErrorInvalidValue;
}

} // namespace ptls_hip
