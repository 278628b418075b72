/*
 * poly1305.h -- Poly1305 (RFC 8439 §2.5) on one 130-bit accumulator, written for host and device: chacha_kernel.hip uses
 * exactly these functions, and tests/test_chacha_poly_native.py compiles them on the host and checks them against the RFC's
 * vectors and a big-integer reference, serially and through the kernel's lane split.
 *
 * Numbers are five 26-bit limbs (value = sum h_i 2^(26 i)) with 64-bit products, the layout of poly1305-donna-32: a
 * product is 25 32 x 32 -> 64 multiply-adds (v_mad_u64_u32 on gfx950), and 2^130 = 5 (mod p) folds the upper half back
 * with a multiplication of the second operand's limbs by 5.  "Carried" below means every limb < 2^26 except h1, which may
 * exceed it by the last carry (< 2^26 + 2^16); poly_mac() accepts a first operand with limbs below 2^28 and a carried
 * second one, and up to five such products may be summed in one PolyWide before poly_carry() (each term is below
 * 2^28 * 5 * 2^26.1 < 2^56.5, 25 of them below 2^61.2).
 */
#pragma once

#include <stdint.h>

/* the function qualifier shared with gf128.h: a host-only build defines it before the include */
#ifndef GF128_FN
#define GF128_FN __host__ __device__ __forceinline__
#endif
#define POLY_FN GF128_FN

namespace ptls_hip {

struct Poly {
    uint32_t h0, h1, h2, h3, h4;
};

/* sums of limb products before the carry */
struct PolyWide {
    uint64_t d0, d1, d2, d3, d4;
};

constexpr uint32_t POLY_MASK26 = 0x3ffffffu;

/* the limbs of a 128-bit little-endian number w0..w3, plus `hibit` (0 or 1) at 2^128 */
POLY_FN Poly poly_limbs(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t hibit)
{
    return Poly{w0 & POLY_MASK26, ((w0 >> 26) | (w1 << 6)) & POLY_MASK26, ((w1 >> 20) | (w2 << 12)) & POLY_MASK26,
                ((w2 >> 14) | (w3 << 18)) & POLY_MASK26, (w3 >> 8) | (hibit << 24)};
}

/* r = the first 16 bytes of the one-time key, clamped (RFC 8439 §2.5: r &= 0x0ffffffc0ffffffc0ffffffc0fffffff) */
POLY_FN Poly poly_clamp_r(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
    return poly_limbs(w0 & 0x0fffffffu, w1 & 0x0ffffffcu, w2 & 0x0ffffffcu, w3 & 0x0ffffffcu, 0);
}

/* a whole 16-byte message block: its bytes as a number, with the high bit 2^128.  A final block of n < 16 bytes is passed
 * to poly_limbs() by the caller as its bytes, the byte 0x01 at position n, zeros above, and hibit 0. */
POLY_FN Poly poly_block(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
    return poly_limbs(w0, w1, w2, w3, 1);
}

POLY_FN Poly poly_zero()
{
    return Poly{0, 0, 0, 0, 0};
}

/* limb-wise sum, no carry: the result's limbs are the sums */
POLY_FN Poly poly_add(Poly a, Poly b)
{
    return Poly{a.h0 + b.h0, a.h1 + b.h1, a.h2 + b.h2, a.h3 + b.h3, a.h4 + b.h4};
}

POLY_FN PolyWide poly_wide_zero()
{
    return PolyWide{0, 0, 0, 0, 0};
}

/* d += a * b (mod 2^130 - 5), uncarried */
POLY_FN void poly_mac(PolyWide &d, Poly a, Poly b)
{
    const uint32_t s1 = b.h1 * 5, s2 = b.h2 * 5, s3 = b.h3 * 5, s4 = b.h4 * 5;
    d.d0 += (uint64_t)a.h0 * b.h0 + (uint64_t)a.h1 * s4 + (uint64_t)a.h2 * s3 + (uint64_t)a.h3 * s2 + (uint64_t)a.h4 * s1;
    d.d1 += (uint64_t)a.h0 * b.h1 + (uint64_t)a.h1 * b.h0 + (uint64_t)a.h2 * s4 + (uint64_t)a.h3 * s3 + (uint64_t)a.h4 * s2;
    d.d2 += (uint64_t)a.h0 * b.h2 + (uint64_t)a.h1 * b.h1 + (uint64_t)a.h2 * b.h0 + (uint64_t)a.h3 * s4 + (uint64_t)a.h4 * s3;
    d.d3 += (uint64_t)a.h0 * b.h3 + (uint64_t)a.h1 * b.h2 + (uint64_t)a.h2 * b.h1 + (uint64_t)a.h3 * b.h0 + (uint64_t)a.h4 * s4;
    d.d4 += (uint64_t)a.h0 * b.h4 + (uint64_t)a.h1 * b.h3 + (uint64_t)a.h2 * b.h2 + (uint64_t)a.h3 * b.h1 + (uint64_t)a.h4 * b.h0;
}

/* the carried form of d (mod 2^130 - 5) */
POLY_FN Poly poly_carry(PolyWide d)
{
    Poly h;
    uint64_t c;
    c = d.d0 >> 26;
    h.h0 = (uint32_t)d.d0 & POLY_MASK26;
    d.d1 += c;
    c = d.d1 >> 26;
    h.h1 = (uint32_t)d.d1 & POLY_MASK26;
    d.d2 += c;
    c = d.d2 >> 26;
    h.h2 = (uint32_t)d.d2 & POLY_MASK26;
    d.d3 += c;
    c = d.d3 >> 26;
    h.h3 = (uint32_t)d.d3 & POLY_MASK26;
    d.d4 += c;
    c = d.d4 >> 26;
    h.h4 = (uint32_t)d.d4 & POLY_MASK26;
    const uint64_t t = (uint64_t)h.h0 + c * 5; /* c < 2^38 */
    h.h0 = (uint32_t)t & POLY_MASK26;
    h.h1 += (uint32_t)(t >> 26);
    return h;
}

/* a * b (mod 2^130 - 5), carried: a's limbs below 2^28, b carried (a power of r, or one) */
POLY_FN Poly poly_mul(Poly a, Poly b)
{
    PolyWide d = poly_wide_zero();
    poly_mac(d, a, b);
    return poly_carry(d);
}

/* the tag: (h mod 2^130 - 5) + s mod 2^128, as four little-endian words; h's limbs below 2^28 */
POLY_FN void poly_finish(Poly h, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t &t0, uint32_t &t1, uint32_t &t2,
                         uint32_t &t3)
{
    uint32_t c;
    /* two carry passes: after the first every limb but h0 is below 2^26, after the second all are */
    for (int pass = 0; pass < 2; ++pass) {
        c = h.h0 >> 26;
        h.h0 &= POLY_MASK26;
        h.h1 += c;
        c = h.h1 >> 26;
        h.h1 &= POLY_MASK26;
        h.h2 += c;
        c = h.h2 >> 26;
        h.h2 &= POLY_MASK26;
        h.h3 += c;
        c = h.h3 >> 26;
        h.h3 &= POLY_MASK26;
        h.h4 += c;
        c = h.h4 >> 26;
        h.h4 &= POLY_MASK26;
        h.h0 += c * 5;
    }
    /* (the first pass leaves a value below 2^130 + 5 * 2^6; if the second pass folds a carry again, what stayed below
     * 2^130 is tiny and h0 + 5 does not overflow its limb: every limb is below 2^26 now and h < 2^130 < 2 p) */
    /* g = h - p = h + 5 - 2^130, taken when it is not negative */
    uint32_t g0 = h.h0 + 5;
    c = g0 >> 26;
    g0 &= POLY_MASK26;
    uint32_t g1 = h.h1 + c;
    c = g1 >> 26;
    g1 &= POLY_MASK26;
    uint32_t g2 = h.h2 + c;
    c = g2 >> 26;
    g2 &= POLY_MASK26;
    uint32_t g3 = h.h3 + c;
    c = g3 >> 26;
    g3 &= POLY_MASK26;
    const uint32_t g4 = h.h4 + c - (1u << 26);
    const uint32_t take_g = (g4 >> 31) ? 0u : 0xffffffffu; /* no borrow: h >= p */
    h.h0 = (h.h0 & ~take_g) | (g0 & take_g);
    h.h1 = (h.h1 & ~take_g) | (g1 & take_g);
    h.h2 = (h.h2 & ~take_g) | (g2 & take_g);
    h.h3 = (h.h3 & ~take_g) | (g3 & take_g);
    h.h4 = (h.h4 & ~take_g) | (g4 & take_g);
    /* h mod 2^128 as four words */
    const uint32_t w0 = h.h0 | (h.h1 << 26);
    const uint32_t w1 = (h.h1 >> 6) | (h.h2 << 20);
    const uint32_t w2 = (h.h2 >> 12) | (h.h3 << 14);
    const uint32_t w3 = (h.h3 >> 18) | (h.h4 << 8);
    uint64_t f = (uint64_t)w0 + s0;
    t0 = (uint32_t)f;
    f = (uint64_t)w1 + s1 + (f >> 32);
    t1 = (uint32_t)f;
    f = (uint64_t)w2 + s2 + (f >> 32);
    t2 = (uint32_t)f;
    f = (uint64_t)w3 + s3 + (f >> 32);
    t3 = (uint32_t)f;
}

/* ---- the lane split of chacha_kernel.hip, as arithmetic (the kernel and the host check share these) ----
 *
 * The tag's polynomial is sum m_i r^(N + 1 - i) over the N blocks m_1 .. m_N.  The record's whole 64-byte ChaCha blocks
 * ("chunks", four Poly1305 blocks each) are dealt to G lanes from the END of the data: with nfull chunks,
 * T = nfull / G + 1 trips and pad = T G - nfull (1 .. G) empty places in front, chunk c sits at place c + pad, and place q
 * belongs to lane q % G in trip q / G.  A lane runs acc = acc r^(4G) + chunk over its trips; the place pad - 1, empty and in
 * trip 0, carries everything hashed before the data (the AAD blocks) as that lane's starting value.  The lanes' sums are then
 * joined as sum_l acc_l r^(4 (G - 1 - l)): stage b multiplies the lanes whose bit b is clear by r^(4 2^b) and adds partner
 * lanes l and l ^ 2^b, so after log2 G stages every lane holds the value of the serial Horner loop over AAD and chunks.
 * What follows the whole chunks (up to four blocks of the last partial chunk, then the length block) is hashed serially. */

/* one chunk's four blocks against r^4, r^3, r^2, r on top of acc * rG: acc <- acc rG + m0 r^4 + m1 r^3 + m2 r^2 + m3 r */
POLY_FN Poly poly_chunk(Poly acc, Poly rG, Poly m0, Poly m1, Poly m2, Poly m3, Poly r1, Poly r2, Poly r3, Poly r4)
{
    PolyWide d = poly_wide_zero();
    poly_mac(d, acc, rG);
    poly_mac(d, m0, r4);
    poly_mac(d, m1, r3);
    poly_mac(d, m2, r2);
    poly_mac(d, m3, r1);
    return poly_carry(d);
}

/* the serial step: (acc + m) r */
POLY_FN Poly poly_step(Poly acc, Poly m, Poly r1)
{
    return poly_mul(poly_add(acc, m), r1);
}

/* stage b of the lane combination, before the partner's value is added: acc times r^(4 2^b) (passed as sq) in the lanes
 * whose bit b is clear, times one in the others (the product also carries their limbs, which the additions widen) */
POLY_FN Poly poly_combine_stage(Poly acc, Poly sq, uint32_t lane, int b)
{
    const bool keep = (lane >> b) & 1u;
    const Poly m{keep ? 1u : sq.h0, keep ? 0u : sq.h1, keep ? 0u : sq.h2, keep ? 0u : sq.h3, keep ? 0u : sq.h4};
    return poly_mul(acc, m);
}

} // namespace ptls_hip
