// The host side of tools/bench_quic_parse.py: the walk and the map lookup of csrc/quic_parse.h compiled for the CPU, doing on
// one core what quic_parse_kernel.hip does on the device (the same entries into the same arrays), so that the two can be
// timed against each other.  Built by the tool with g++ -O2 -shared.
#include <cstddef>
#include <cstdint>
#include <cstring>
#define GF128_FN static inline
#include "ptls_hip.h"
#include "quic_parse.h"
using namespace ptls_hip;

extern "C" {

// fills table[0 .. size) (zeroed here) with count CIDs at a 20-byte stride; size = a power of two >= 2 * count
void quic_parse_host_map(QuicCidEntry *table, uint32_t size, const uint8_t *cids, const uint8_t *lens, const uint32_t *conns,
                         size_t count)
{
    std::memset(table, 0, (size_t)size * sizeof(QuicCidEntry));
    for (size_t i = 0; i < count; ++i)
        quic_cid_set(table, size, cids + 20 * i, lens[i], conns[i], [](uint32_t) {});
}

// the entries of dgrams[0 .. n) in buf into pkts / info; returns their number
size_t quic_parse_host(const ptls_hip_quic_datagram_t *dgrams, size_t n, const uint8_t *buf, uint32_t short_cid_len,
                       uint32_t max_per_dgram, uint32_t require_fixed_bit, const QuicCidEntry *table, uint32_t size,
                       ptls_hip_quic_packet_t *pkts, ptls_hip_quic_pktinfo_t *info)
{
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        const ptls_hip_quic_datagram_t dg = dgrams[i];
        const uint8_t *d = buf + dg.off;
        at += quic_walk_datagram(d, dg.len, short_cid_len, max_per_dgram, require_fixed_bit,
                                 [=](uint32_t k, uint32_t pos, const QuicWalk &w, bool more) {
            uint32_t conn = QP_NO_CONN;
            if (w.status == QP_OK)
                conn = quic_cid_lookup(table, size, d + pos + w.dcid_off, w.dcid_len);
            ptls_hip_quic_packet_t p;
            p.pkt_off = dg.off + pos;
            p.data_off = dg.off + pos + w.pn_offset + 1;
            p.pn = 0;
            p.pkt_len = w.pkt_len;
            p.key = p.hp_key = conn;
            p.pn_offset = (uint16_t)w.pn_offset;
            p.pn_len = 0;
            p.flags = 0;
            pkts[at + k] = p;
            ptls_hip_quic_pktinfo_t f = {};
            f.dgram = (uint32_t)i;
            f.version = w.version;
            f.conn = conn;
            f.token_len = w.token_len;
            f.dcid_off = (uint16_t)w.dcid_off;
            f.scid_off = (uint16_t)w.scid_off;
            f.token_off = (uint16_t)w.token_off;
            f.dcid_len = (uint8_t)w.dcid_len;
            f.scid_len = (uint8_t)w.scid_len;
            f.type = (uint8_t)w.type;
            f.status = (uint8_t)w.status;
            f.flags = more ? 1 : 0;
            info[at + k] = f;
        });
    }
    return at;
}
}
