/*
 * quic_tx.h -- what a send call gives a request: its packet number, the encoded length of that number, the header bytes, the
 * key generation and the refusals (RFC 9000 §12.3, §17.1, §17.3.1, A.2; RFC 9001 §6; include/ptls_hip.h 2l),
 * written for host and device like quic_track.h and quic_phase.h: quic_tx_kernel.hip runs exactly these functions, and
 * tests/test_quic_tx_native.py compiles them on the host and checks them against the plain-Python model
 * (tests/quic_tx_ref.py).
 *
 * A request's number is its connection's next_pn BEFORE the call plus its distance from the head of its run; the state after
 * the call is that next_pn plus the run's length.  Everything is integer arithmetic on values read before the call, so the
 * outcome does not depend on the order in which the requests are looked at.
 */
#pragma once

#include <stdint.h>

#include "ptls_hip.h"

/* the function qualifier shared with gf128.h, quic.h and quic_rx.h: a host-only build defines it before the include */
#ifndef GF128_FN
#define GF128_FN __host__ __device__ __forceinline__
#endif
#define QTX_FN GF128_FN

namespace ptls_hip {

constexpr uint32_t QTX_NO_POS = 0xffffffffu; /* "no first run yet" in the per-connection scratch; positions are below it */
constexpr uint64_t QTX_PN_END = (uint64_t)1 << 62;
constexpr uint32_t QTX_MAX_DCID = 20, QTX_MAX_PKT = 65535, QTX_TAG = 16;

/* what a send call knows on the host and every request is held against */
struct QuicTxLimits {
    uint64_t in_len, buf_len; /* bytes of the payload buffer and of the packet buffer */
    uint32_t nconn;           /* min(count, stride, slots of hp_ks): a connection at or above it is TX_NO_CONN */
    uint32_t stride;          /* generation g of connection c: key slot c + stride * (g % 3) */
    uint32_t min_pn_len;      /* params.pn_len: 0 (minimal) or 1..4 (at least that many bytes) */
    uint32_t has_rx_phase;    /* 0: no d_rx_phase, the generation is the send state's own */
};

/* the j-th request's number in a run whose head is d requests in front of it; the sum saturates at UINT64_MAX (any value from
 * 2^62 on is refused alike) */
QTX_FN uint64_t quic_tx_pn(uint64_t next_pn, uint64_t d)
{
    return next_pn > UINT64_MAX - d ? UINT64_MAX : next_pn + d;
}

/* RFC 9000 §17.1: the smallest length in max(1, min_len) .. 4 that holds more than twice the range of unacknowledged numbers
 * (num_unacked < 2^(8 L - 1)), 0 when none does.  A.2's examples: largest_acked 0xabe8b3, pn 0xac5c02 -> 2; pn 0xace8fe -> 3.
 * pn < 2^62 and largest_acked == UINT64_MAX or < pn. */
QTX_FN uint32_t quic_tx_pn_len(uint64_t pn, uint64_t largest_acked, uint32_t min_len)
{
    const uint64_t num_unacked = largest_acked == UINT64_MAX ? pn + 1 : pn - largest_acked;
    uint32_t len = 0;
#pragma unroll
    for (uint32_t l = 4; l >= 1; --l)
        if (l >= min_len && num_unacked < ((uint64_t)1 << (8 * l - 1)))
            len = l;
    return len;
}

/* the generation a connection sends under: its own, or the receive side's where that is ahead (a peer's key update that
 * rx_keyphase_commit committed, RFC 9001 §6.2) */
QTX_FN uint32_t quic_tx_gen(uint32_t gen, bool has_rx, uint32_t rx_gen)
{
    return has_rx && rx_gen > gen ? rx_gen : gen;
}

/* the AEAD key slot of generation gen of connection c (quic_phase.h's layout) */
QTX_FN uint32_t quic_tx_slot(uint32_t conn, uint32_t stride, uint32_t gen)
{
    return conn + stride * (gen % 3u);
}

/* a short header's first byte: fixed bit, spin bit, reserved bits 0, Key Phase bit, packet-number length (RFC 9000 §17.3.1) */
QTX_FN uint32_t quic_tx_first_byte(uint32_t flags, uint32_t gen, uint32_t pn_len)
{
    return 0x40u | ((flags & 1u) << 5) | ((gen & 1u) << 2) | (pn_len - 1u);
}

/* byte k (0 .. pn_len - 1) of the packet-number field: the low pn_len bytes of pn, big-endian */
QTX_FN uint32_t quic_tx_pn_byte(uint64_t pn, uint32_t pn_len, uint32_t k)
{
    return (uint32_t)(pn >> (8 * (pn_len - 1u - k))) & 0xffu;
}

struct QuicTxVerdict {
    uint32_t status;  /* PTLS_HIP_QUIC_TX_* */
    uint32_t pn_len;  /* 1..4 when sent */
    uint32_t pkt_len; /* 0 unless sent */
};

/* Rules 4 to 6 for a request of a numbered run: pn = its number, dcid_len and largest_acked its connection's.  No
 * intermediate wraps for any request or state bytes. */
QTX_FN QuicTxVerdict quic_tx_judge(const ptls_hip_quic_txreq_t &r, uint64_t pn, uint64_t largest_acked, uint32_t dcid_len,
                                   const QuicTxLimits &l)
{
    if (pn >= QTX_PN_END || (largest_acked != UINT64_MAX && largest_acked >= pn))
        return QuicTxVerdict{PTLS_HIP_QUIC_TX_PN, 0, 0};
    const uint32_t pn_len = quic_tx_pn_len(pn, largest_acked, l.min_pn_len);
    if (pn_len == 0)
        return QuicTxVerdict{PTLS_HIP_QUIC_TX_PN, 0, 0};
    if (dcid_len > QTX_MAX_DCID)
        return QuicTxVerdict{PTLS_HIP_QUIC_TX_RANGE, 0, 0};
    const uint64_t body = (uint64_t)pn_len + r.len; /* the header-protection sample is 16 bytes from 4 behind the number's start */
    const uint64_t pkt_len = 1u + (uint64_t)dcid_len + body + QTX_TAG;
    if (body < 4 || pkt_len > QTX_MAX_PKT)
        return QuicTxVerdict{PTLS_HIP_QUIC_TX_RANGE, 0, 0};
    if (r.data_off > l.in_len || r.len > l.in_len - r.data_off)
        return QuicTxVerdict{PTLS_HIP_QUIC_TX_RANGE, 0, 0};
    if (r.pkt_off > l.buf_len || pkt_len > l.buf_len - r.pkt_off)
        return QuicTxVerdict{PTLS_HIP_QUIC_TX_RANGE, 0, 0};
    return QuicTxVerdict{PTLS_HIP_QUIC_TX_SENT, pn_len, (uint32_t)pkt_len};
}

/* The wave-per-record kernel's plan is a stable order by decreasing 16-byte block count, as quic_rx.h's: a sent payload is
 * below 65 535 bytes, so the ascending key 4095 - (len >> 4) has 12 bits */
QTX_FN uint32_t quic_tx_sort_key(uint32_t len)
{
    return 4095u - (len >> 4);
}

/* the sent packet's descriptors, as ptls_hip_quic_seal_batch's quic_records makes them for a host-written header */
QTX_FN ptls_hip_quic_packet_t quic_tx_packet(const ptls_hip_quic_txreq_t &r, uint64_t pn, uint32_t pn_len, uint32_t pkt_len,
                                             uint32_t dcid_len, uint32_t slot)
{
    ptls_hip_quic_packet_t p{};
    p.pkt_off = r.pkt_off;
    p.data_off = r.data_off;
    p.pn = pn;
    p.pkt_len = pkt_len;
    p.key = slot;
    p.hp_key = r.conn;
    p.pn_offset = (uint16_t)(1u + dcid_len);
    p.pn_len = (uint8_t)pn_len;
    p.flags = 0;
    return p;
}

QTX_FN ptls_hip_record_t quic_tx_record(const ptls_hip_quic_packet_t &p)
{
    ptls_hip_record_t r{};
    r.aad_off = p.pkt_off;
    r.aad_len = (uint32_t)p.pn_offset + p.pn_len;
    r.len = p.pkt_len - r.aad_len - QTX_TAG;
    r.seq = p.pn;
    r.key = p.key;
    r.flags = 0;
    r.in_off = p.data_off;
    r.out_off = p.pkt_off + r.aad_len;
    return r;
}

/* the header-protection descriptor of the packet at compacted position `at`: the sample at pn_offset + 4, the mask at 16 at */
QTX_FN ptls_hip_supp_t quic_tx_supp(const ptls_hip_quic_packet_t &p, uint64_t at)
{
    return ptls_hip_supp_t{p.pkt_off + p.pn_offset + 4u, 16 * at, p.hp_key, PTLS_HIP_SUPP_ENABLE};
}

/* what the select pass sums over the sent packets, in this order in device memory (integers: any order of addition) */
enum { QTX_STAT_COUNT = 0, QTX_STAT_BYTES, QTX_STAT_BLOCKS64, QTX_NSTATS };

} // namespace ptls_hip
