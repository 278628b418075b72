/*
 * ctr_window.h -- rounds 1-2 of an AES counter block from per-record and per-window constants.
 * Compiles for the device (batch_kernel.h) and, with no HIP at all, on the host (tests/host_check/ctr_window_check.cpp
 * checks it against plain FIPS-197 rounds on the CPU).
 *
 * The AES input of data block c of a record is nonce (12 bytes) || counter (4 bytes, big-endian, c + 2).  While the
 * counter stays below 2^16 its bytes are 00 00 hi lo, so:
 *   after round 1   column 0 takes counter byte 15 (lo), column 1 takes counter byte 14 (hi), columns 2 and 3 are fixed
 *                   per record;
 *   after round 2   every column is (a per-record constant) ^ (two lookups, one of round-1 column 0 and one of column 1).
 * Column 1 of round 1, and with it the four round-2 lookups that read it, changes only with counter byte 14: they are the
 * same for the 256 consecutive counters of one WINDOW (window = counter >> 8).  CtrConst holds what is fixed per record,
 * CtrWin what is fixed per (record, window): a block then costs 1 lookup in round 1 and 4 in round 2 (instead of 2 + 8),
 * and a window's constants cost 5 lookups once.
 *
 * Words are little-endian state columns (byte k of word c = state row k, column c), `cw` is the counter word as it sits
 * in the state (bswap32 of the counter), rk the round keys as such words.  TAB is the T-table accessor:
 *   tab.template t0<K>(x) = T0[byte K of x],  tab.template t2<K>(x) = rotl16(T0[byte K of x]),
 * T0[v] = (2s, s, s, 3s) little-endian, s = S-box(v); T1 = rotl8(T0), T3 = rotl8(T2).
 */
#pragma once

#include <stdint.h>

/* the function qualifier, as in gf128.h: device + host under hipcc; a host-only build defines GF128_FN (e.g. inline) */
#ifndef GF128_FN
#define GF128_FN __host__ __device__ __forceinline__
#endif
#define CTRW_FN GF128_FN

namespace ptls_hip {

CTRW_FN uint32_t ctrw_rotl8(uint32_t x)
{
    return (x << 8) | (x >> 24); /* one v_alignbit_b32 on the device */
}

/* per record */
struct CtrConst {
    uint32_t k10, k11; /* round-1 columns 0, 1 without their counter-byte term */
    uint32_t k20, k21, k22, k23; /* round-2 columns without the terms from round-1 columns 0 and 1 */
    uint32_t r03;      /* round key 0 word 3 (the counter word's whitening) */
};

/* per (record, window): the round-2 constants with the terms from round-1 column 1 folded in */
struct CtrWin {
    uint32_t w0, w1, w2, w3;
};

template <class TAB>
CTRW_FN CtrConst ctr_const(const TAB &tab, const uint32_t *rk, uint32_t n0, uint32_t n1, uint32_t n2)
{
    const uint32_t s0 = n0 ^ rk[0], s1 = n1 ^ rk[1], s2 = n2 ^ rk[2], s3 = rk[3]; /* counter bytes 12,13 = 0 */
    CtrConst c;
    c.r03 = rk[3];
    /* round 1: t_c = T0[s_c.b0] ^ T1[s_{c+1}.b1] ^ T2[s_{c+2}.b2] ^ T3[s_{c+3}.b3] ^ rk1_c */
    c.k10 = tab.template t0<0>(s0) ^ ctrw_rotl8(tab.template t0<1>(s1)) ^ tab.template t2<2>(s2) ^ rk[4]; /* - T3[s3.b3] */
    c.k11 = tab.template t0<0>(s1) ^ ctrw_rotl8(tab.template t0<1>(s2)) ^ ctrw_rotl8(tab.template t2<3>(s0)) ^ rk[5]; /* - T2[s3.b2] */
    const uint32_t t2 = tab.template t0<0>(s2) ^ ctrw_rotl8(tab.template t0<1>(s3)) ^ tab.template t2<2>(s0) ^
                        ctrw_rotl8(tab.template t2<3>(s1)) ^ rk[6];
    const uint32_t t3 = tab.template t0<0>(s3) ^ ctrw_rotl8(tab.template t0<1>(s0)) ^ tab.template t2<2>(s1) ^
                        ctrw_rotl8(tab.template t2<3>(s2)) ^ rk[7];
    /* round 2 constant parts (terms reading t2, t3) */
    c.k20 = tab.template t2<2>(t2) ^ ctrw_rotl8(tab.template t2<3>(t3)) ^ rk[8];
    c.k21 = ctrw_rotl8(tab.template t0<1>(t2)) ^ tab.template t2<2>(t3) ^ rk[9];
    c.k22 = tab.template t0<0>(t2) ^ ctrw_rotl8(tab.template t0<1>(t3)) ^ rk[10];
    c.k23 = tab.template t0<0>(t3) ^ ctrw_rotl8(tab.template t2<3>(t2)) ^ rk[11];
    return c;
}

/* the window of a block counter, and whether a lane that steps its counter by `step` (<= 256) per iteration has entered
 * a new window with `ctr` (ctr - step lies in the window before): the iteration in which its CtrWin must be refreshed */
CTRW_FN uint32_t ctr_window_of(uint32_t ctr)
{
    return ctr >> 8;
}

CTRW_FN bool ctr_window_crossed(uint32_t ctr, uint32_t step)
{
    return (ctr & 255u) < step;
}

/* round-1 column 1 of counter word cw (1 lookup), and the term of round-2 column W that reads it (1 lookup each) */
template <class TAB>
CTRW_FN uint32_t ctr_window_t1(const TAB &tab, uint32_t k11, uint32_t r03, uint32_t cw)
{
    return k11 ^ tab.template t2<2>(cw ^ r03);
}

template <int W, class TAB>
CTRW_FN uint32_t ctr_window_term(const TAB &tab, uint32_t t1)
{
    static_assert(W >= 0 && W < 4, "state column");
    return W == 0 ? ctrw_rotl8(tab.template t0<1>(t1))
         : W == 1 ? tab.template t0<0>(t1)
         : W == 2 ? ctrw_rotl8(tab.template t2<3>(t1))
                  : tab.template t2<2>(t1);
}

/* the constants of cw's window: the record's round-2 constants with the four terms folded in (5 lookups) */
template <class TAB>
CTRW_FN CtrWin ctr_window(const TAB &tab, const CtrConst &c, uint32_t cw)
{
    const uint32_t t1 = ctr_window_t1(tab, c.k11, c.r03, cw);
    CtrWin w;
    w.w0 = c.k20 ^ ctr_window_term<0>(tab, t1);
    w.w1 = c.k21 ^ ctr_window_term<1>(tab, t1);
    w.w2 = c.k22 ^ ctr_window_term<2>(tab, t1);
    w.w3 = c.k23 ^ ctr_window_term<3>(tab, t1);
    return w;
}

/* Column W of the constants of the window of t1n from that (w) of the window of t1o, without the record's round-2
 * constants: the old round-1 column 1's term is XORed out and the new one's in (2 lookups).  A whole step (2 + 8 lookups)
 * needs only k11 and r03 of CtrConst, which is what the kernel's loop keeps in registers; the same window on both sides
 * changes nothing. */
template <int W, class TAB>
CTRW_FN uint32_t ctr_window_step_col(const TAB &tab, uint32_t w, uint32_t t1o, uint32_t t1n)
{
    return w ^ ctr_window_term<W>(tab, t1o) ^ ctr_window_term<W>(tab, t1n);
}

template <class TAB>
CTRW_FN CtrWin ctr_window_step(const TAB &tab, uint32_t k11, uint32_t r03, const CtrWin &w, uint32_t cwo, uint32_t cwn)
{
    const uint32_t to = ctr_window_t1(tab, k11, r03, cwo), tn = ctr_window_t1(tab, k11, r03, cwn);
    CtrWin n;
    n.w0 = ctr_window_step_col<0>(tab, w.w0, to, tn);
    n.w1 = ctr_window_step_col<1>(tab, w.w1, to, tn);
    n.w2 = ctr_window_step_col<2>(tab, w.w2, to, tn);
    n.w3 = ctr_window_step_col<3>(tab, w.w3, to, tn);
    return n;
}

/* a block's rounds 1-2 in the window form, issue and finish apart (the kernel runs them a segment apart):
 * round 1 = one lookup m -> column 0; round 2 = four lookups m[4] of column 0 -> the state */
template <class TAB>
CTRW_FN uint32_t ctrw_r1_issue(const TAB &tab, const CtrConst &c, uint32_t cw)
{
    return tab.template t2<3>(cw ^ c.r03);
}

CTRW_FN uint32_t ctrw_r1_finish(const CtrConst &c, uint32_t m)
{
    return c.k10 ^ ctrw_rotl8(m);
}

template <class TAB>
CTRW_FN void ctrw_r2_issue(const TAB &tab, uint32_t t0, uint32_t (&m)[4])
{
    m[0] = tab.template t0<0>(t0);
    m[1] = tab.template t2<3>(t0);
    m[2] = tab.template t2<2>(t0);
    m[3] = tab.template t0<1>(t0);
}

CTRW_FN void ctrw_r2_finish(const CtrWin &w, const uint32_t (&m)[4], uint32_t (&s)[4])
{
    s[0] = w.w0 ^ m[0];
    s[1] = w.w1 ^ ctrw_rotl8(m[1]);
    s[2] = w.w2 ^ m[2];
    s[3] = w.w3 ^ ctrw_rotl8(m[3]);
}

/* the four pieces in a row: the state of counter word cw after round 2, w = the constants of cw's window */
template <class TAB>
CTRW_FN void ctr_rounds12_window(const TAB &tab, const CtrConst &c, const CtrWin &w, uint32_t cw, uint32_t (&s)[4])
{
    uint32_t m[4];
    ctrw_r2_issue(tab, ctrw_r1_finish(c, ctrw_r1_issue(tab, c, cw)), m);
    ctrw_r2_finish(w, m, s);
}

} // namespace ptls_hip
