/*
 * chacha_runs.h -- the piece map of chacha_runs_kernel.hip, as arithmetic for host and device (the kernel uses exactly these
 * functions; tests/native/chacha_runs_check.cpp checks them on the host for every group width and block count).
 *
 * The deal of poly1305.h stays: G lanes share a record, its nfull whole 64-byte blocks sit at places pad .. T G - 1
 * (T = nfull / G + 1 trips, pad = T G - nfull), block c at place c + pad.  What differs from chacha_kernel.hip is which lane
 * touches which bytes.  A trip's G places are 4 G pieces of 16 bytes, contiguous in the record; load (and store)
 * instruction j = 0 .. 3 has lane l move piece j G + l, so one instruction moves one contiguous run of 16 G bytes per group.
 * Piece j G + l is quarter l & 3 of the trip's place j (G / 4) + (l >> 2): the four lanes of quad q hold, after the four
 * loads, a 4 x 4 matrix [lane a][instruction j] = quarter a of place j (G / 4) + q.  Its transpose gives lane 4 q + a the
 * four quarters, in order, of place a (G / 4) + q.  So lane l owns, in every trip, the place
 *     lambda(l) = (l & 3) (G / 4) + (l >> 2)
 * of the trip, and lambda takes the part of l wherever the deal speaks of a lane: the empty places of trip 0, the AAD's place,
 * and the lane combination, before which the accumulators move to the lanes the combination expects (runs_acc_source).
 *
 * The transpose is two butterfly stages inside a quad (partner lane l ^ 1, then l ^ 2): in stage b, of each register pair
 * (j, j | 1 << b) a lane keeps the register whose bit b equals its own bit b and trades the other for the partner's
 * (runs_send / runs_recv).  It is its own inverse: the stores run it again and write the same runs.
 */
#pragma once

#include <stdint.h>

#include "poly1305.h"

namespace ptls_hip {

/* the place, within a trip, of the block lane l (0 .. G - 1) owns; G = 4: l itself */
POLY_FN uint32_t runs_lambda(uint32_t G, uint32_t l)
{
    return (l & 3u) * (G / 4) + (l >> 2);
}

/* the lane that owns place m of a trip: runs_lambda(G, runs_lambda_inv(G, m)) == m */
POLY_FN uint32_t runs_lambda_inv(uint32_t G, uint32_t m)
{
    return (m % (G / 4)) * 4 + m / (G / 4);
}

/* the lane combination wants the sum of place m in lane m: lane m takes it from this lane */
POLY_FN uint32_t runs_acc_source(uint32_t G, uint32_t m)
{
    return runs_lambda_inv(G, m);
}

/* trips and empty leading places of a record with nfull whole blocks */
POLY_FN uint32_t runs_trips(uint32_t G, uint32_t nfull)
{
    return nfull / G + 1;
}

POLY_FN uint32_t runs_pad(uint32_t G, uint32_t nfull)
{
    return runs_trips(G, nfull) * G - nfull;
}

/* the byte offset, in the record's data, of the 16-byte piece lane l moves with instruction j of trip t, or -1: the piece
 * lies before the record's first byte (trip 0 only) and is neither loaded nor stored.  Never past 64 nfull. */
POLY_FN int64_t runs_piece_off(uint32_t G, uint32_t nfull, uint32_t t, uint32_t j, uint32_t l)
{
    const int64_t off = ((int64_t)t * G - (int64_t)runs_pad(G, nfull)) * 64 + (int64_t)(j * G + l) * 16;
    return off >= 0 ? off : -1;
}

/* where that piece sits after the exchange: the lane, and the slot (the quarter of that lane's block) */
POLY_FN uint32_t runs_piece_lane(uint32_t l, uint32_t j)
{
    return (l & ~3u) | j;
}

POLY_FN uint32_t runs_piece_slot(uint32_t l)
{
    return l & 3u;
}

/* whether lane l has a block in trip t, and which (the ChaCha counter is block + 1) */
POLY_FN bool runs_has_block(uint32_t G, uint32_t nfull, uint32_t t, uint32_t l)
{
    return t * G + runs_lambda(G, l) >= runs_pad(G, nfull);
}

POLY_FN uint32_t runs_block(uint32_t G, uint32_t nfull, uint32_t t, uint32_t l)
{
    return t * G + runs_lambda(G, l) - runs_pad(G, nfull);
}

/* stage b (0, 1) of the quad transpose on the register pair (lo, hi) = (j, j | 1 << b): the word lane l gives to lane
 * l ^ (1 << b), and what it does with the word it gets */
POLY_FN uint32_t runs_send(uint32_t lo, uint32_t hi, uint32_t l, int b)
{
    return (l >> b) & 1u ? lo : hi;
}

POLY_FN void runs_recv(uint32_t &lo, uint32_t &hi, uint32_t l, int b, uint32_t got)
{
    if ((l >> b) & 1u)
        lo = got;
    else
        hi = got;
}

} // namespace ptls_hip
