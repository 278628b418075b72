/*
 * quic.h -- the header arithmetic of QUIC packet protection (RFC 9001 §5.4.1, RFC 9000 Appendix A.3), written for host and
 * device: quic_kernel.hip runs exactly these functions on the packets in device memory, and tests/test_quic_native.py
 * compiles them on the host and checks them against the plain-Python reference (tests/quic_ref.py).  A mask travels as two
 * little-endian words (bytes 0..3 and 4..7 of the 16-byte header-protection block; QUIC uses bytes 0..4), never as an
 * array a lane could index at run time.
 */
#pragma once

#include <stdint.h>

/* the function qualifier shared with gf128.h and chacha20.h: a host-only build defines it before the include */
#ifndef GF128_FN
#define GF128_FN __host__ __device__ __forceinline__
#endif
#define QUIC_FN GF128_FN

namespace ptls_hip {

/* RFC 9000 Appendix A.3 (DecodePacketNumber) with expected = largest_pn + 1: the packet number closest to `expected` whose
 * low 8 * pn_len bits are `truncated`.  pn_len is 1..4.  The RFC's comparisons are over the integers; here they are
 * arranged so that no unsigned intermediate wraps, for any 64-bit `expected`. */
QUIC_FN uint64_t quic_decode_pn(uint64_t expected, uint64_t truncated, uint32_t pn_len)
{
    const uint64_t win = (uint64_t)1 << (8 * pn_len), hwin = win >> 1, mask = win - 1;
    const uint64_t candidate = (expected & ~mask) | (truncated & mask);
    if (expected >= hwin && candidate <= expected - hwin && candidate < ((uint64_t)1 << 62) - win)
        return candidate + win;
    if (candidate > expected && candidate - expected > hwin && candidate >= win)
        return candidate - win;
    return candidate;
}

/* the bits of the first byte under header protection (RFC 9001 §5.4.1): the low four of a long header (0x80 set: reserved
 * bits and packet-number length), the low five of a short one (also the key phase) */
QUIC_FN uint32_t quic_first_byte_bits(uint32_t first)
{
    return (first & 0x80u) != 0 ? 0x0fu : 0x1fu;
}

/* mask byte k (0..4) of the words m0 = bytes 0..3, m1 = bytes 4..7 */
QUIC_FN uint32_t quic_mask_byte(uint32_t m0, uint32_t m1, int k)
{
    return k < 4 ? (m0 >> (8 * k)) & 0xffu : m1 & 0xffu;
}

/* Send side: protects the header at hdr in place.  The first byte and the pn_len (1..4) packet-number bytes at
 * hdr + pn_offset are the only bytes read or written. */
QUIC_FN void quic_protect_header(uint8_t *hdr, uint32_t pn_offset, uint32_t pn_len, uint32_t m0, uint32_t m1)
{
    const uint32_t first = hdr[0];
    hdr[0] = (uint8_t)(first ^ (m0 & quic_first_byte_bits(first)));
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if ((uint32_t)j < pn_len)
            hdr[pn_offset + j] = (uint8_t)(hdr[pn_offset + j] ^ quic_mask_byte(m0, m1, 1 + j));
}

/* Receive side, in two steps so that a kernel can issue the header's loads together with the sample's, before the mask is
 * known.  quic_load_header reads hdr[0] and the four bytes hdr[pn_offset .. pn_offset + 4), whatever the packet-number
 * length turns out to be: they lie inside the packet, because the 16-byte sample starts at pn_offset + 4. */
struct QuicHeaderBytes {
    uint32_t first, b0, b1, b2, b3;
};

QUIC_FN QuicHeaderBytes quic_load_header(const uint8_t *hdr, uint32_t pn_offset)
{
    return QuicHeaderBytes{hdr[0], hdr[pn_offset], hdr[pn_offset + 1], hdr[pn_offset + 2], hdr[pn_offset + 3]};
}

/* With `masked`, removes the mask from the first byte, reads the packet-number length from it, removes the mask from that
 * many packet-number bytes and writes those 1 + pn_len bytes back to hdr (nothing else is written; without `masked`,
 * nothing at all).  Returns pn_len (1..4) and the truncated packet number in *truncated. */
QUIC_FN uint32_t quic_unprotect_header(uint8_t *hdr, uint32_t pn_offset, QuicHeaderBytes h, bool masked, uint32_t m0,
                                       uint32_t m1, uint64_t *truncated)
{
    uint32_t first = h.first;
    if (masked) {
        first ^= m0 & quic_first_byte_bits(first); /* (the form bit 0x80 is never masked) */
        hdr[0] = (uint8_t)first;
    }
    const uint32_t pn_len = (first & 3u) + 1u;
    const uint32_t b[4] = {h.b0, h.b1, h.b2, h.b3};
    uint64_t t = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if ((uint32_t)j < pn_len) {
            uint32_t v = b[j];
            if (masked) {
                v ^= quic_mask_byte(m0, m1, 1 + j);
                hdr[pn_offset + j] = (uint8_t)v;
            }
            t = (t << 8) | v;
        }
    *truncated = t;
    return pn_len;
}

} // namespace ptls_hip
