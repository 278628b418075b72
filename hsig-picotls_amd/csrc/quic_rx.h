/*
 * quic_rx.h -- the per-packet arithmetic of the device-side receive step (include/ptls_hip.h 2i), written
 * for host and device like quic.h and quic_parse.h: quic_rx_kernel.hip runs exactly these functions on the descriptors in
 * device memory, and tests/test_quic_rx_native.py compiles them on the host and checks them against the plain-Python model
 * (tests/quic_rx_ref.py).  The select rule (which parsed entries an open call takes), the provisional record lengths the
 * planner's statistics are taken over (pn_len = 1, as quic_records makes them: the packet-number length sits under header
 * protection), and the sort key of the sparse kernel's plan order.
 */
#pragma once

#include <stdint.h>

#include "ptls_hip.h"

/* the function qualifier shared with gf128.h, quic.h and quic_parse.h: a host-only build defines it before the include */
#ifndef GF128_FN
#define GF128_FN __host__ __device__ __forceinline__
#endif
#define QRX_FN GF128_FN

namespace ptls_hip {

/* what an open call knows on the host and every descriptor is held against */
struct QuicRxLimits {
    uint64_t buf_len, out_len;  /* bytes of the packet buffer and of the output buffer */
    uint64_t nslots, hp_nslots; /* key slots of the AEAD and of the header-protection keyset */
    uint32_t type_mask;         /* bit t: packets of PTLS_HIP_QUIC_TYPE_t are taken */
    uint32_t has_info;          /* 0: no info records (ptls_hip_quic_rx_set_packets without them), the mask is ignored */
};

/* The refusals of quic_packet_fault (pn_offset != 0, the header-protection sample inside the packet) and of the open call
 * (key slots inside their keysets: PTLS_HIP_QUIC_NO_CONN is outside any), per packet, and what a host caller guarantees by
 * passing buffers: the packet inside the packet buffer, the plaintext area of pkt_len - pn_offset - 17 bytes (the pn_len = 1
 * size, the largest the kernel can write) inside the output buffer.  No intermediate wraps for any descriptor bytes. */
QRX_FN bool quic_rx_selectable(const ptls_hip_quic_packet_t &p, uint32_t type, const QuicRxLimits &l)
{
    if (p.pn_offset == 0)
        return false;
    if (p.pkt_len < (uint32_t)p.pn_offset + 20u || p.pkt_len > 65535u)
        return false;
    if (p.pkt_off > l.buf_len || p.pkt_len > l.buf_len - p.pkt_off)
        return false;
    const uint32_t area = p.pkt_len - (uint32_t)p.pn_offset - 17u;
    if (p.data_off > l.out_len || area > l.out_len - p.data_off)
        return false;
    if (p.key >= l.nslots || p.hp_key >= l.hp_nslots)
        return false;
    if (l.has_info != 0 && (type > 31u || ((l.type_mask >> type) & 1u) == 0))
        return false;
    return true;
}

/* the provisional record of a selected packet: AAD = pn_offset + 1 header bytes, then the payload up to the tag */
QRX_FN uint32_t quic_rx_len(const ptls_hip_quic_packet_t &p)
{
    return p.pkt_len - (uint32_t)p.pn_offset - 17u;
}

/* GHASH elements ceil(aad / 16) + ceil(len / 16) + 1 (choose_lanes' sum) */
QRX_FN uint32_t quic_rx_ghash_elems(const ptls_hip_quic_packet_t &p)
{
    return ((uint32_t)p.pn_offset + 1u + 15u) / 16u + (quic_rx_len(p) + 15u) / 16u + 1u;
}

/* The sparse kernel's plan is a stable order by decreasing 16-byte block count (build_chunks).  pkt_len <= 65535 bounds the
 * count by 4094, so the ascending key 4095 - (len >> 4) has 12 bits: two radix digits of QRX_DIGIT_BITS. */
constexpr uint32_t QRX_DIGIT_BITS = 6, QRX_DIGITS = 1u << QRX_DIGIT_BITS, QRX_KEY_MAX = 4095;
QRX_FN uint32_t quic_rx_sort_key(const ptls_hip_quic_packet_t &p)
{
    return QRX_KEY_MAX - (quic_rx_len(p) >> 4);
}

/* what the stats pass sums over the selected packets, in this order in device memory (all integers: the sums do not depend
 * on the order of addition) */
enum { QRX_STAT_GHASH = 0, QRX_STAT_BLOCKS64, QRX_STAT_RUNS, QRX_STAT_MAX16, QRX_STAT_COUNT, QRX_NSTATS };

} // namespace ptls_hip
