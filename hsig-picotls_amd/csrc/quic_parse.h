/*
 * quic_parse.h -- the arithmetic of parsing QUIC datagrams (include/ptls_hip.h 2h), written for host and
 * device like quic.h: quic_parse_kernel.hip runs exactly these functions on datagrams in device memory, quic_parse.cpp runs
 * the connection-ID map's hash and probe loop on its host mirror, and tests/test_quic_parse_native.py compiles all of it
 * with g++ and checks it against the plain-Python reference (tests/quic_parse_ref.py).  Walk state lives in scalars; there
 * is no local array a lane could index at run time.
 *
 * The hard rule: nothing here reads a byte at or past the end of the datagram.  A packet is described by the pointer `p` to
 * its first byte and by `rest`, the bytes from there to the datagram's end; every load of p[k] stands behind a check k < rest.
 *
 * The walk of one packet (quic_walk_packet; rest >= 1), in this order:
 *   short header (first & 0x80 == 0): type ONE_RTT.  Fixed bit (below) -> BAD_FIXED_BIT.  pn_offset = 1 + short_cid_len;
 *     rest < pn_offset + 20 -> TOO_SHORT.  Else DCID at 1, short_cid_len bytes, and the packet takes the rest of the datagram
 *     (RFC 9000 §12.2).
 *   long header: rest < 5 -> TRUNCATED (type NONE); version = big-endian word at 1.  Its type: version 0 ->
 *     VERSION_NEGOTIATION; 1 -> the v1 bits (first >> 4) & 3 = Initial 0, 0-RTT 1, Handshake 2, Retry 3; 0x6b3343cf -> the v2
 *     bits of RFC 9369 §3.2 = Retry 0, Initial 1, 0-RTT 2, Handshake 3; anything else -> UNKNOWN_VERSION.
 *     Known version: fixed bit -> BAD_FIXED_BIT.
 *     DCID length at 5 (rest < 6 -> TRUNCATED); known version and length > 20 -> BAD_CID_LEN; the DCID bytes and the SCID
 *     length byte behind them must lie in the datagram (6 + dcid_len >= rest -> TRUNCATED), then the DCID is recorded; SCID
 *     length > 20 under a known version -> BAD_CID_LEN; 7 + dcid_len + scid_len > rest -> TRUNCATED, then the SCID is recorded.
 *     Version 0, an unknown version and Retry end here: status OK, pn_offset 0 (they carry no packet protection), the rest
 *     of the datagram.
 *     Initial: the token-length varint (does not fit -> TRUNCATED), the token (longer than what is left -> TRUNCATED), then
 *     recorded.  Initial, 0-RTT, Handshake: the Length varint (does not fit -> TRUNCATED); pn_offset = the byte behind it;
 *     Length < 20 -> TOO_SHORT; Length > rest - pn_offset -> TRUNCATED; pkt_len = pn_offset + Length.
 *   Fixed bit: with require_fixed_bit != 0, first & 0x40 == 0 is BAD_FIXED_BIT; with 0 the bit is not looked at (RFC 9287).
 *   Every status but OK ends the datagram: pkt_len = rest, pn_offset = 0; the fields recorded before the error stand, the
 *   others are 0.  An entry is openable iff pn_offset != 0, and then pkt_len >= pn_offset + 20.
 */
#pragma once

#include <stdint.h>

#ifndef GF128_FN
#define GF128_FN __host__ __device__ __forceinline__
#endif
#define QUIC_FN GF128_FN

namespace ptls_hip {

/* the values of include/ptls_hip.h PTLS_HIP_QUIC_TYPE_* / _STATUS_* (quic_parse.cpp asserts the equality) */
constexpr uint32_t QP_INITIAL = 0, QP_ZERO_RTT = 1, QP_HANDSHAKE = 2, QP_RETRY = 3, QP_ONE_RTT = 4, QP_VERSION_NEGOTIATION = 5,
                   QP_UNKNOWN_VERSION = 6, QP_NONE = 7;
constexpr uint32_t QP_OK = 0, QP_TRUNCATED = 1, QP_TOO_SHORT = 2, QP_BAD_CID_LEN = 3, QP_BAD_FIXED_BIT = 4;
constexpr uint32_t QP_NO_CONN = 0xffffffffu;
constexpr uint32_t QP_V1 = 0x00000001u, QP_V2 = 0x6b3343cfu;
constexpr uint32_t QP_MAX_CID = 20, QP_MIN_PROTECTED = 20; /* packet number + payload + tag: 4 + 16 (the sample's reach) */

/* RFC 9000 §16: the varint at p[pos], of 1, 2, 4 or 8 bytes, all of which must lie below `rest`.  Non-minimal encodings
 * decode like any other.  False (nothing else read) when it does not fit. */
QUIC_FN bool quic_varint(const uint8_t *p, uint32_t pos, uint32_t rest, uint64_t *value, uint32_t *next)
{
    if (pos >= rest)
        return false;
    const uint32_t b0 = p[pos];
    const uint32_t len = 1u << (b0 >> 6);
    if (len > rest - pos)
        return false;
    uint64_t v = b0 & 0x3fu;
    for (uint32_t j = 1; j < len; ++j)
        v = (v << 8) | p[pos + j];
    *value = v;
    *next = pos + len;
    return true;
}

struct QuicWalk {
    uint32_t status, type, version;
    uint32_t dcid_off, dcid_len, scid_off, scid_len, token_off, token_len; /* offsets from the packet's first byte */
    uint32_t pn_offset, pkt_len;
};

/* the packet that starts at p with `rest` (1..65535) bytes to the datagram's end; the rules are in the header comment */
QUIC_FN QuicWalk quic_walk_packet(const uint8_t *p, uint32_t rest, uint32_t short_cid_len, uint32_t require_fixed_bit)
{
    QuicWalk w{};
    w.status = QP_TRUNCATED; /* every early return below that sets nothing else is a truncation */
    w.type = QP_NONE;
    w.pkt_len = rest;
    const uint32_t first = p[0];
    const bool fixed_bad = require_fixed_bit != 0 && (first & 0x40u) == 0;
    if ((first & 0x80u) == 0) {
        w.type = QP_ONE_RTT;
        if (fixed_bad) {
            w.status = QP_BAD_FIXED_BIT;
            return w;
        }
        if (rest < 1 + short_cid_len + QP_MIN_PROTECTED) {
            w.status = QP_TOO_SHORT;
            return w;
        }
        w.dcid_off = 1;
        w.dcid_len = short_cid_len;
        w.pn_offset = 1 + short_cid_len;
        w.status = QP_OK;
        return w;
    }
    if (rest < 5)
        return w;
    const uint32_t version = (uint32_t)p[1] << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 8 | (uint32_t)p[4];
    w.version = version;
    const bool known = version == QP_V1 || version == QP_V2;
    const uint32_t bits = (first >> 4) & 3u;
    w.type = version == 0 ? QP_VERSION_NEGOTIATION : version == QP_V1 ? bits : version == QP_V2 ? (bits + 3u) & 3u : QP_UNKNOWN_VERSION;
    if (known && fixed_bad) {
        w.status = QP_BAD_FIXED_BIT;
        return w;
    }
    if (rest < 6)
        return w;
    const uint32_t dl = p[5];
    if (known && dl > QP_MAX_CID) {
        w.status = QP_BAD_CID_LEN;
        return w;
    }
    if (6 + dl >= rest)
        return w;
    w.dcid_off = 6;
    w.dcid_len = dl;
    const uint32_t sl = p[6 + dl];
    if (known && sl > QP_MAX_CID) {
        w.status = QP_BAD_CID_LEN;
        return w;
    }
    uint32_t pos = 7 + dl + sl;
    if (pos > rest)
        return w;
    w.scid_off = 7 + dl;
    w.scid_len = sl;
    if (!known || w.type == QP_RETRY) {
        w.status = QP_OK;
        return w;
    }
    uint64_t v;
    if (w.type == QP_INITIAL) {
        if (!quic_varint(p, pos, rest, &v, &pos) || v > rest - pos)
            return w;
        w.token_off = pos;
        w.token_len = (uint32_t)v;
        pos += (uint32_t)v;
    }
    if (!quic_varint(p, pos, rest, &v, &pos))
        return w;
    if (v < QP_MIN_PROTECTED) {
        w.status = QP_TOO_SHORT;
        return w;
    }
    if (v > rest - pos)
        return w;
    w.pn_offset = pos;
    w.pkt_len = pos + (uint32_t)v;
    w.status = QP_OK;
    return w;
}

/* the packet-number space of an openable type: Initial 0, Handshake 1, 0-RTT and 1-RTT 2 (RFC 9000 §12.3) */
QUIC_FN uint32_t quic_pn_space(uint32_t type)
{
    return type == QP_INITIAL ? 0u : type == QP_HANDSHAKE ? 1u : 2u;
}

/* ---- the connection-ID map: open addressing, linear probing, 32-byte entries, a power-of-two table at load <= 0.5 ---- */

struct QuicCidEntry {
    uint8_t cid[QP_MAX_CID];
    uint8_t len, used;
    uint16_t pad0;
    uint32_t conn;
    uint32_t pad1;
};
static_assert(sizeof(QuicCidEntry) == 32, "a CID map entry is 32 bytes");

/* FNV-1a over the length and every byte of the CID, then the 32-bit finalizer of MurmurHash3 (the table index takes the low bits) */
QUIC_FN uint32_t quic_cid_hash(const uint8_t *cid, uint32_t len)
{
    uint32_t h = (2166136261u ^ len) * 16777619u;
    for (uint32_t j = 0; j < len; ++j)
        h = (h ^ cid[j]) * 16777619u;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

QUIC_FN bool quic_cid_equal(const QuicCidEntry *e, const uint8_t *cid, uint32_t len)
{
    if (e->len != len)
        return false;
    bool same = true;
    for (uint32_t j = 0; j < len; ++j)
        same = same && e->cid[j] == cid[j];
    return same;
}

/* The probe loop of lookup and insert alike: from the CID's home slot forward, at most `size` steps (size = a power of two),
 * to the entry that holds the CID (true, *slot = its index) or to the first free entry (false, *slot = its index; `size`
 * when the table is full, which the load bound rules out).  Reads only; len <= 20. */
QUIC_FN bool quic_cid_probe(const QuicCidEntry *table, uint32_t size, const uint8_t *cid, uint32_t len, uint32_t *slot)
{
    const uint32_t mask = size - 1;
    uint32_t i = quic_cid_hash(cid, len) & mask;
    for (uint32_t step = 0; step < size; ++step, i = (i + 1) & mask) {
        const QuicCidEntry *e = table + i;
        if (e->used == 0) {
            *slot = i;
            return false;
        }
        if (quic_cid_equal(e, cid, len)) {
            *slot = i;
            return true;
        }
    }
    *slot = size;
    return false;
}

/* the connection of a CID, or QP_NO_CONN (also for a null table or a length above 20) */
QUIC_FN uint32_t quic_cid_lookup(const QuicCidEntry *table, uint32_t size, const uint8_t *cid, uint32_t len)
{
    uint32_t slot;
    if (table == nullptr || len > QP_MAX_CID || !quic_cid_probe(table, size, cid, len, &slot))
        return QP_NO_CONN;
    return table[slot].conn;
}

/* The two updates of the host mirror (quic_parse.cpp; the device only reads).  Both call touched(slot) for every entry they
 * change, so that the host uploads exactly those. */

/* insert or replace; the table must have a free entry.  True when the CID is new. */
template <class Touched>
QUIC_FN bool quic_cid_set(QuicCidEntry *table, uint32_t size, const uint8_t *cid, uint32_t len, uint32_t conn, Touched touched)
{
    uint32_t slot;
    const bool found = quic_cid_probe(table, size, cid, len, &slot);
    QuicCidEntry *e = table + slot;
    if (!found) {
        *e = QuicCidEntry{};
        for (uint32_t j = 0; j < len; ++j)
            e->cid[j] = cid[j];
        e->len = (uint8_t)len;
        e->used = 1;
    }
    e->conn = conn;
    touched(slot);
    return !found;
}

/* backward-shift delete, no tombstones: every later entry of the cluster whose home slot does not lie cyclically in (hole, j]
 * moves into the hole, which then is where it was.  True when the CID was there. */
template <class Touched>
QUIC_FN bool quic_cid_remove(QuicCidEntry *table, uint32_t size, const uint8_t *cid, uint32_t len, Touched touched)
{
    const uint32_t mask = size - 1;
    uint32_t i;
    if (!quic_cid_probe(table, size, cid, len, &i))
        return false;
    for (uint32_t j = (i + 1) & mask, step = 1; step < size && table[j].used != 0; j = (j + 1) & mask, ++step) {
        const uint32_t home = quic_cid_hash(table[j].cid, table[j].len) & mask;
        const bool stays = i <= j ? (i < home && home <= j) : (i < home || home <= j);
        if (stays)
            continue;
        table[i] = table[j];
        touched(i);
        i = j;
    }
    table[i] = QuicCidEntry{};
    touched(i);
    return true;
}

/* ---- the entries of one datagram, in wire order (the count pass and the write pass run the same loop) ---- */

/* Calls emit(k, pos, walk, more) for entry k = 0, 1, ... of the datagram at d[0 .. len): the packet starts at d + pos;
 * `more` is set on entry max_per_dgram - 1 when bytes are left behind it (they are dropped).  Returns the number of entries:
 * 0 for an empty datagram, else 1 .. max_per_dgram. */
template <class Emit>
QUIC_FN uint32_t quic_walk_datagram(const uint8_t *d, uint32_t len, uint32_t short_cid_len, uint32_t max_per_dgram,
                                    uint32_t require_fixed_bit, Emit emit)
{
    uint32_t pos = 0, k = 0;
    while (pos < len && k < max_per_dgram) {
        const QuicWalk w = quic_walk_packet(d + pos, len - pos, short_cid_len, require_fixed_bit);
        const uint32_t next = pos + w.pkt_len; /* <= len: pkt_len <= rest */
        emit(k, pos, w, k + 1 == max_per_dgram && next < len);
        pos = next;
        ++k;
    }
    return k;
}

} // namespace ptls_hip
