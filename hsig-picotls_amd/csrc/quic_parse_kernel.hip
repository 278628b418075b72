/*
 * quic_parse_kernel.hip -- QUIC datagrams parsed on the device (include/ptls_hip.h 2h).
 *
 * The output is dense and ordered, so it takes three steps: quic_parse_count_kernel walks every datagram (one thread each)
 * and writes its number of entries; quic_parse_scan_kernel turns one level of counts into exclusive prefix sums within spans
 * of QP_SCAN_SPAN and the span totals into the next level (one launch per level: no workgroup ever waits for another);
 * quic_parse_write_kernel walks every datagram again and writes its entries at the scanned offset, with the connection-ID
 * lookup and the expected packet number.  The walk is quic_parse.h's, the same code in both passes: the headers are one or
 * two 128-byte lines per packet, still in the L2 for the second pass, whereas staging max_per_dgram entries of 72 bytes per
 * datagram would write and read more than the headers hold.  Placement uses no atomics: the order is the input's.
 *
 * Exact bytes: every load from the packet buffer is a single byte below the datagram's end (quic_parse.h), at any alignment.
 * Walk state stays in scalars (no private segment); the CID compare reads the packet and the table entry directly.
 */
#include <hip/hip_runtime.h>

#include "internal.h"
#include "quic_parse.h"
#include "quic_scan.h"

namespace ptls_hip {

constexpr int QP_WG = 256;
constexpr int QP_SCAN_ITEMS = 8;
static_assert(QP_WG * QP_SCAN_ITEMS == (int)QP_SCAN_SPAN, "one scan workgroup covers one span");

__global__ void __launch_bounds__(QP_WG) quic_parse_count_kernel(const QuicParseArgs a)
{
    for (uint64_t i = (uint64_t)blockIdx.x * QP_WG + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * QP_WG) {
        const ptls_hip_quic_datagram_t dg = a.dgrams[i];
        a.scan.l0[i] = quic_walk_datagram(a.buf + dg.off, dg.len, a.short_cid_len, a.max_per_dgram, a.require_fixed_bit,
                                     [](uint32_t, uint32_t, const QuicWalk &, bool) {});
    }
}

__global__ void __launch_bounds__(QP_WG) quic_parse_scan_kernel(uint32_t *__restrict__ v, uint32_t n, uint32_t *__restrict__ sums)
{
    __shared__ uint32_t s[QP_WG];
    const uint32_t tid = threadIdx.x;
    const uint32_t nspans = (uint32_t)(((uint64_t)n + QP_SCAN_SPAN - 1) / QP_SCAN_SPAN);
    for (uint32_t span = blockIdx.x; span < nspans; span += gridDim.x) { /* (uniform per workgroup: the barriers are safe) */
        const uint64_t base = (uint64_t)span * QP_SCAN_SPAN + (uint64_t)tid * QP_SCAN_ITEMS;
        uint32_t x[QP_SCAN_ITEMS], mine = 0;
#pragma unroll
        for (int j = 0; j < QP_SCAN_ITEMS; ++j) {
            x[j] = base + j < n ? v[base + j] : 0u;
            mine += x[j];
        }
        s[tid] = mine;
        __syncthreads();
#pragma unroll
        for (uint32_t d = 1; d < (uint32_t)QP_WG; d <<= 1) { /* Hillis-Steele over the 256 thread sums */
            const uint32_t t = tid >= d ? s[tid - d] : 0u;
            __syncthreads();
            s[tid] += t;
            __syncthreads();
        }
        uint32_t run = s[tid] - mine;
#pragma unroll
        for (int j = 0; j < QP_SCAN_ITEMS; ++j) {
            if (base + j < n)
                v[base + j] = run;
            run += x[j];
        }
        if (tid == QP_WG - 1)
            sums[span] = s[tid];
        __syncthreads(); /* s is reused by the next span */
    }
}

__global__ void __launch_bounds__(QP_WG) quic_parse_write_kernel(const QuicParseArgs a)
{
    for (uint64_t i = (uint64_t)blockIdx.x * QP_WG + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * QP_WG) {
        const ptls_hip_quic_datagram_t dg = a.dgrams[i];
        const uint32_t at = scan_at(a.scan, i);
        const uint8_t *d = a.buf + dg.off;
        quic_walk_datagram(d, dg.len, a.short_cid_len, a.max_per_dgram, a.require_fixed_bit,
                           [=](uint32_t k, uint32_t pos, const QuicWalk &w, bool more) {
            uint32_t conn = QP_NO_CONN;
            if (w.status == QP_OK)
                conn = quic_cid_lookup(a.table, a.table_size, d + pos + w.dcid_off, w.dcid_len);
            uint64_t pn = 0;
            if (w.pn_offset != 0 && a.expected_pn != nullptr && conn != QP_NO_CONN) {
                const uint64_t e = (uint64_t)conn * 3 + quic_pn_space(w.type);
                if (e < a.expected_count)
                    pn = a.expected_pn[e];
            }
            ptls_hip_quic_packet_t p;
            p.pkt_off = dg.off + pos;
            p.data_off = dg.off + pos + w.pn_offset + 1;
            p.pn = pn;
            p.pkt_len = w.pkt_len;
            p.key = conn;
            p.hp_key = conn;
            p.pn_offset = (uint16_t)w.pn_offset;
            p.pn_len = 0;
            p.flags = 0;
            a.pkts[(uint64_t)at + k] = p;
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
            f.flags = more ? (uint8_t)PTLS_HIP_QUIC_INFO_MORE : (uint8_t)0;
            a.info[(uint64_t)at + k] = f;
        });
    }
}

int launch_quic_parse_count(const QuicParseArgs &a, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_parse_count_kernel, dim3(grid), dim3(QP_WG), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

int launch_quic_parse_scan(uint32_t *v, uint32_t n, uint32_t *sums, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_parse_scan_kernel, dim3(grid), dim3(QP_WG), 0, static_cast<hipStream_t>(stream), v, n, sums);
    return (int)hipGetLastError();
}

int launch_quic_parse_write(const QuicParseArgs &a, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_parse_write_kernel, dim3(grid), dim3(QP_WG), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

} // namespace ptls_hip
