/*
 * quic_ack.h -- the ACK frame of one packet-number space entry (RFC 9000 §19.3, type 0x02, no ECN counts; varints of §16;
 * include/ptls_hip.h 2m), written for host and device like quic_track.h and quic_tx.h:
 * quic_ack_kernel.hip runs exactly these functions, and tests/test_quic_ack_native.py compiles them on the host and checks
 * them against the plain-Python model (tests/quic_ack_ref.py).  Integers only.
 *
 * The entry is quic_track.h's (next, window): bit k of window = packet number next - 1 - k has been accepted.  Bits at
 * k >= next name no packet number and are masked.  A run is a maximal stretch of consecutive set bits, counted from bit 0
 * upwards: run 0 starts at bit 0 (the largest accepted number), every further run is one ACK range behind a gap.
 */
#pragma once

#include <stdint.h>

#include "ptls_hip.h"
#include "quic_parse.h"

#define QAK_FN QUIC_FN

namespace ptls_hip {

constexpr uint32_t QAK_MAX_RANGES = 31;            /* a 64-bit window has at most 32 runs */
constexpr uint64_t QAK_VARINT_END = 1ull << 62;    /* varints hold values below it */

/* the encoded length of v < 2^62 */
QAK_FN uint32_t quic_ack_vl(uint64_t v)
{
    return v < 64 ? 1u : v < 16384 ? 2u : v < (1u << 30) ? 4u : 8u;
}

/* the window with the bits that name no packet number cleared (next != 0) */
QAK_FN uint64_t quic_ack_masked(uint64_t next, uint64_t window)
{
    return next >= 64 ? window : window & (((uint64_t)1 << next) - 1);
}

/* the status of a list entry; in_table: conn < count, and only then (next, window) were read */
QAK_FN uint32_t quic_ack_status(bool in_table, uint64_t next, uint64_t window)
{
    if (!in_table)
        return PTLS_HIP_QUIC_ACK_NO_CONN;
    if (next == 0)
        return PTLS_HIP_QUIC_ACK_EMPTY;
    if (next > QAK_VARINT_END || (window & 1) == 0)
        return PTLS_HIP_QUIC_ACK_STATE;
    return PTLS_HIP_QUIC_ACK_OK;
}

/* ACK Range Count of a masked window with bit 0 set: its runs behind run 0, the newest max_ranges of them */
QAK_FN uint32_t quic_ack_ranges(uint64_t w, uint32_t max_ranges)
{
    const uint32_t runs = (uint32_t)__builtin_popcountll(w & ~(w << 1)); /* a run starts where a set bit has none below it */
    const uint32_t keep = max_ranges < QAK_MAX_RANGES ? max_ranges : QAK_MAX_RANGES;
    return runs - 1 < keep ? runs - 1 : keep;
}

/* the frame length of an ACK_OK entry: 5 .. PTLS_HIP_QUIC_ACK_MAX */
QAK_FN uint32_t quic_ack_len(uint64_t next, uint64_t window, uint64_t ack_delay, uint32_t max_ranges)
{
    return 1 + quic_ack_vl(next - 1) + quic_ack_vl(ack_delay) + 2 + 2 * quic_ack_ranges(quic_ack_masked(next, window), max_ranges);
}

/* the status, and the frame length or 0, of list entry `conn` */
QAK_FN uint32_t quic_ack_judge(const ptls_hip_quic_pnspace_t *spaces, uint64_t count, uint32_t space, uint32_t conn, uint64_t ack_delay,
                               uint32_t max_ranges, ptls_hip_quic_pnspace_t *st, uint32_t *len)
{
    const bool in_table = conn < count;
    st->next = 0, st->window = 0;
    if (in_table)
        *st = spaces[3 * (uint64_t)conn + space];
    const uint32_t status = quic_ack_status(in_table, st->next, st->window);
    *len = status == PTLS_HIP_QUIC_ACK_OK ? quic_ack_len(st->next, st->window, ack_delay, max_ranges) : 0;
    return status;
}

/* the number of set bits from bit 0 upwards, and of clear bits from bit 0 upwards (x != 0) */
QAK_FN uint32_t quic_ack_ones(uint64_t x)
{
    return ~x == 0 ? 64u : (uint32_t)__builtin_ctzll(~x);
}

QAK_FN uint32_t quic_ack_zeros(uint64_t x)
{
    return (uint32_t)__builtin_ctzll(x);
}

/* x moved down by 1 .. 64 bits */
QAK_FN uint64_t quic_ack_drop(uint64_t x, uint32_t by)
{
    return by >= 64 ? 0 : x >> by;
}

/* v < 2^62 as a minimal varint at p: the bytes stored one by one, most significant first; returns their number */
QAK_FN uint32_t quic_ack_put(uint8_t *p, uint64_t v)
{
    const uint32_t n = quic_ack_vl(v);
    const uint64_t x = v | (uint64_t)(n == 1 ? 0 : n == 2 ? 1 : n == 4 ? 2 : 3) << (8 * n - 2);
    for (uint32_t k = 0; k < n; ++k)
        p[k] = (uint8_t)(x >> (8 * (n - 1 - k)));
    return n;
}

/* the frame of an ACK_OK entry at p, every field stored as it is produced; returns its length (quic_ack_len's) */
QAK_FN uint32_t quic_ack_write(uint8_t *p, uint64_t next, uint64_t window, uint64_t ack_delay, uint32_t max_ranges)
{
    uint64_t rest = quic_ack_masked(next, window);
    const uint32_t r = quic_ack_ranges(rest, max_ranges);
    uint32_t at = 0;
    p[at++] = 0x02;
    at += quic_ack_put(p + at, next - 1);
    at += quic_ack_put(p + at, ack_delay);
    p[at++] = (uint8_t)r;
    uint32_t run = quic_ack_ones(rest);
    p[at++] = (uint8_t)(run - 1);
    rest = quic_ack_drop(rest, run);
    for (uint32_t i = 0; i < r; ++i) { /* (r further runs exist: rest != 0 and its bit 0 is clear) */
        const uint32_t gap = quic_ack_zeros(rest);
        p[at++] = (uint8_t)(gap - 1);
        rest >>= gap;
        run = quic_ack_ones(rest);
        p[at++] = (uint8_t)(run - 1);
        rest = quic_ack_drop(rest, run);
    }
    return at;
}

/* the send request of the frame of list entry `conn` that is the call's pos-th frame */
QAK_FN ptls_hip_quic_txreq_t quic_ack_request(uint64_t in_off, uint32_t frame_off, uint64_t pkt_base, uint64_t pkt_stride, uint32_t pos,
                                              uint32_t conn, uint32_t len)
{
    ptls_hip_quic_txreq_t r;
    r.data_off = in_off + frame_off;
    r.pkt_off = pkt_base + (uint64_t)pos * pkt_stride;
    r.conn = conn;
    r.len = len;
    return r;
}

} // namespace ptls_hip
