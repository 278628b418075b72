/*
 * quic_tx_kernel.hip -- the send object's passes in front of and behind the record kernel: packet numbers assigned, headers
 * written and send keys chosen on the device (include/ptls_hip.h 2l).  The rule is quic_tx.h's.
 *
 *   quic_tx_heads_kernel   one thread per request: the 0 / 1 flag "this request begins a run" (and the zeroing of the sums);
 *                          a head lowers its connection's scratch word to its position (32-bit integer atomicMin: the
 *                          connection's first run, whatever the order)
 *   (the scan levels of quic_parse_kernel.hip turn the flags into run indices)
 *   quic_tx_runs_kernel    one thread per request: a head stores its position at its run's index
 *   quic_tx_select_kernel  one thread per request: the rule, from the state as it was before the call: status, packet number
 *                          and packet length into the caller's arrays, the 0 / 1 flag "sent", and the sums the lane choice
 *                          and the report need (wave reduction, then integer atomics)
 *   (the scan levels again: the flags into compacted positions, in request order)
 *   quic_tx_build_kernel   one thread per request: a sent packet's header bytes into the packet buffer, and at its position
 *                          the packed descriptor, the record, the header-protection descriptor and the sort key
 *   quic_tx_apply_kernel   one thread per request, a launch of its own behind every pass that reads the state: the head of a
 *                          connection's first run moves next_pn on by the run's length, stores the generation used and resets
 *                          the scratch word
 *   quic_tx_order_kernel   AES only, behind the radix passes of quic_rx_kernel.hip: the records in plan order, and the
 *                          wave-per-record kernel's single chunk
 *
 * Every loop is a grid stride over the requests or over at most 20 connection-ID bytes.  No kernel has a private segment or
 * uses LDS; the header bytes are single-byte stores, so nothing outside a sent packet's header is written.
 */
#include <hip/hip_runtime.h>

#include "internal.h"
#include "quic_scan.h"
#include "quic_tx.h"

namespace ptls_hip {

constexpr int QTX_WG = 256;

namespace {

__device__ __forceinline__ bool is_head(const QuicTxArgs &a, uint64_t j, uint32_t conn)
{
    return j == 0 || a.reqs[j - 1].conn != conn;
}

/* the generation connection c sends under in this call: from the state before it */
__device__ __forceinline__ uint32_t gen_of(const QuicTxArgs &a, uint32_t c)
{
    const bool has_rx = a.rx_phase != nullptr;
    return quic_tx_gen(a.conns[c].gen, has_rx, has_rx ? a.rx_phase[c].gen : 0u);
}

} // namespace

__global__ void __launch_bounds__(QTX_WG) quic_tx_heads_kernel(const QuicTxArgs a, const QuicTxLimits lim)
{
    if (blockIdx.x == 0 && threadIdx.x < QTX_NSTATS)
        a.stats[threadIdx.x] = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * QTX_WG + threadIdx.x; j < a.n; j += (uint64_t)gridDim.x * QTX_WG) {
        const uint32_t conn = a.reqs[j].conn;
        const bool head = is_head(a, j, conn);
        a.runs.l0[j] = head ? 1u : 0u;
        if (head && conn < lim.nconn)
            atomicMin(a.first + conn, (uint32_t)j);
    }
}

__global__ void __launch_bounds__(QTX_WG) quic_tx_runs_kernel(const QuicTxArgs a)
{
    for (uint64_t j = (uint64_t)blockIdx.x * QTX_WG + threadIdx.x; j < a.n; j += (uint64_t)gridDim.x * QTX_WG) {
        if (is_head(a, j, a.reqs[j].conn)) /* (the flag itself is gone: the scan wrote the prefix over it) */
            a.run_start[scan_at(a.runs, j)] = (uint32_t)j;
        if (j + 1 == a.n)
            a.run_start[*a.nruns] = a.n;
    }
}

__global__ void __launch_bounds__(QTX_WG) quic_tx_select_kernel(const QuicTxArgs a, const QuicTxLimits lim)
{
    uint64_t count = 0, bytes = 0, blocks = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * QTX_WG + threadIdx.x; j < a.n; j += (uint64_t)gridDim.x * QTX_WG) {
        const ptls_hip_quic_txreq_t r = a.reqs[j];
        QuicTxVerdict v{PTLS_HIP_QUIC_TX_NO_CONN, 0, 0};
        uint64_t pn = UINT64_MAX;
        if (r.conn < lim.nconn) {
            const uint32_t run = scan_at(a.runs, j) - (is_head(a, j, r.conn) ? 0u : 1u);
            const uint32_t h = a.run_start[run];
            if (a.first[r.conn] != h) {
                v.status = PTLS_HIP_QUIC_TX_SPLIT;
            } else {
                pn = quic_tx_pn(a.conns[r.conn].next_pn, j - h);
                v = quic_tx_judge(r, pn, a.conns[r.conn].largest_acked, a.conns[r.conn].dcid_len, lim);
            }
        }
        a.status[j] = v.status;
        a.pn_out[j] = pn;
        a.pkt_len[j] = v.pkt_len;
        const bool sent = v.status == PTLS_HIP_QUIC_TX_SENT;
        a.sent.l0[j] = sent ? 1u : 0u;
        if (sent) {
            ++count;
            bytes += v.pkt_len;
            blocks += r.len / 64u;
        }
    }
    /* (every lane of the wave arrives here: the workgroup is whole waves and the loop has no early return) */
    count = wave_sum(count);
    bytes = wave_sum(bytes);
    blocks = wave_sum(blocks);
    if ((threadIdx.x & 63) == 0 && count != 0) {
        atomicAdd(reinterpret_cast<unsigned long long *>(a.stats + QTX_STAT_COUNT), (unsigned long long)count);
        atomicAdd(reinterpret_cast<unsigned long long *>(a.stats + QTX_STAT_BYTES), (unsigned long long)bytes);
        atomicAdd(reinterpret_cast<unsigned long long *>(a.stats + QTX_STAT_BLOCKS64), (unsigned long long)blocks);
    }
}

__global__ void __launch_bounds__(QTX_WG) quic_tx_build_kernel(const QuicTxArgs a, const QuicTxLimits lim)
{
    for (uint64_t j = (uint64_t)blockIdx.x * QTX_WG + threadIdx.x; j < a.n; j += (uint64_t)gridDim.x * QTX_WG) {
        if (a.status[j] != PTLS_HIP_QUIC_TX_SENT) /* (written by the select pass, a launch ago) */
            continue;
        const ptls_hip_quic_txreq_t r = a.reqs[j];
        const uint32_t at = scan_at(a.sent, j);
        if (at >= a.n)
            continue; /* (never: at most n requests are sent) */
        const uint64_t pn = a.pn_out[j];
        const uint32_t pkt_len = a.pkt_len[j];
        const uint32_t dcid_len = a.conns[r.conn].dcid_len; /* (<= 20: the request was sent) */
        const uint32_t pn_len = pkt_len - 1u - dcid_len - r.len - QTX_TAG;
        const uint32_t gen = gen_of(a, r.conn);
        uint8_t *hdr = a.pkt + r.pkt_off;
        hdr[0] = (uint8_t)quic_tx_first_byte(a.conns[r.conn].flags, gen, pn_len);
#pragma unroll
        for (uint32_t k = 0; k < QTX_MAX_DCID; ++k)
            if (k < dcid_len)
                hdr[1u + k] = a.conns[r.conn].dcid[k];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (k < pn_len)
                hdr[1u + dcid_len + k] = (uint8_t)quic_tx_pn_byte(pn, pn_len, k);
        const ptls_hip_quic_packet_t p = quic_tx_packet(r, pn, pn_len, pkt_len, dcid_len, quic_tx_slot(r.conn, lim.stride, gen));
        a.packed[at] = p;
        a.recs[at] = quic_tx_record(p);
        a.supp[at] = quic_tx_supp(p, at);
        a.keys[at] = quic_tx_sort_key(r.len);
    }
}

__global__ void __launch_bounds__(QTX_WG) quic_tx_apply_kernel(const QuicTxArgs a, const QuicTxLimits lim)
{
    for (uint64_t j = (uint64_t)blockIdx.x * QTX_WG + threadIdx.x; j < a.n; j += (uint64_t)gridDim.x * QTX_WG) {
        const uint32_t conn = a.reqs[j].conn;
        if (conn >= lim.nconn || !is_head(a, j, conn) || a.first[conn] != (uint32_t)j)
            continue;
        /* the one thread of the call that owns connection conn */
        const uint32_t run = scan_at(a.runs, j);
        const uint32_t len = a.run_start[run + 1u] - (uint32_t)j;
        const uint32_t gen = gen_of(a, conn);
        a.conns[conn].next_pn = quic_tx_pn(a.conns[conn].next_pn, len);
        a.conns[conn].gen = gen;
        a.first[conn] = QTX_NO_POS;
    }
}

__global__ void __launch_bounds__(QTX_WG) quic_tx_order_kernel(const ptls_hip_record_t *__restrict__ recs,
                                                               const uint32_t *__restrict__ order, const uint32_t m,
                                                               ptls_hip_record_t *__restrict__ recs_ord, Chunk *chunk)
{
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *chunk = Chunk{0u, m, 0xffffffffu, 0u};
    for (uint64_t t = (uint64_t)blockIdx.x * QTX_WG + threadIdx.x; t < m; t += (uint64_t)gridDim.x * QTX_WG)
        recs_ord[t] = recs[min(order[t], m - 1u)]; /* (a permutation of 0 .. m - 1: the bound holds a stray read inside) */
}

static unsigned grid_check(unsigned grid)
{
    return grid != 0 ? grid : 1;
}

int launch_quic_tx_heads(const QuicTxArgs &a, const QuicTxLimits &lim, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_tx_heads_kernel, dim3(grid_check(grid)), dim3(QTX_WG), 0, static_cast<hipStream_t>(stream), a, lim);
    return (int)hipGetLastError();
}

int launch_quic_tx_runs(const QuicTxArgs &a, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_tx_runs_kernel, dim3(grid_check(grid)), dim3(QTX_WG), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

int launch_quic_tx_select(const QuicTxArgs &a, const QuicTxLimits &lim, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_tx_select_kernel, dim3(grid_check(grid)), dim3(QTX_WG), 0, static_cast<hipStream_t>(stream), a, lim);
    return (int)hipGetLastError();
}

int launch_quic_tx_build(const QuicTxArgs &a, const QuicTxLimits &lim, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_tx_build_kernel, dim3(grid_check(grid)), dim3(QTX_WG), 0, static_cast<hipStream_t>(stream), a, lim);
    return (int)hipGetLastError();
}

int launch_quic_tx_apply(const QuicTxArgs &a, const QuicTxLimits &lim, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_tx_apply_kernel, dim3(grid_check(grid)), dim3(QTX_WG), 0, static_cast<hipStream_t>(stream), a, lim);
    return (int)hipGetLastError();
}

int launch_quic_tx_order(const ptls_hip_record_t *recs, const uint32_t *order, uint32_t m, ptls_hip_record_t *recs_ord, Chunk *chunk,
                         unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_tx_order_kernel, dim3(grid_check(grid)), dim3(QTX_WG), 0, static_cast<hipStream_t>(stream), recs, order, m,
                       recs_ord, chunk);
    return (int)hipGetLastError();
}

} // namespace ptls_hip
