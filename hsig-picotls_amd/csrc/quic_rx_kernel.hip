/*
 * quic_rx_kernel.hip -- the device-side receive step between the parse and the open kernels (include/ptls_hip.h 2i,
 * DESIGN.md §10.4): which of the parsed entries an open call takes, their dense copy, the sums the lane choice needs, and
 * the sparse kernel's plan order.
 *
 *   quic_rx_select_kernel   one thread per entry: the rule of quic_rx.h as a 0 / 1 flag (and the zeroing of the sums)
 *   (the scan levels of quic_parse_kernel.hip turn the flags into positions)
 *   quic_rx_compact_kernel  one thread per entry: a selected entry's index, descriptor and sort key at its position.  No
 *                           atomics: the output is in entry order
 *   quic_rx_stats_kernel    the integer sums over the packed descriptors (wave reduction, then integer atomics: the result
 *                           does not depend on the order of addition), and the sparse kernel's single chunk
 *   quic_rx_hist_kernel / quic_rx_scatter_kernel
 *                           one stable LSD radix pass of 6 bits over tiles of QRX_TILE positions: the [digit][tile] counts,
 *                           then, after their exclusive scan, the placement.  A position's rank among the equal digits of its
 *                           wave's round comes from ballots; rounds and waves are ordered through an LDS table of per-wave
 *                           counts.  Every load and store of the passes is a coalesced 4-byte access except the gather of the
 *                           second pass's keys.
 *
 * No kernel has a private segment: per-round values live under compile-time indices of unrolled loops.
 */
#include <hip/hip_runtime.h>

#include "internal.h"
#include "quic_rx.h"
#include "quic_scan.h"

namespace ptls_hip {

constexpr int QRX_WG = 256;
constexpr int QRX_WAVES = QRX_WG / 64;
constexpr int QRX_ROUNDS = (int)QRX_TILE / QRX_WG;
static_assert(QRX_WAVES * QRX_ROUNDS * 64 == (int)QRX_TILE, "a tile is four waves of four rounds");
static_assert(QRX_DIGITS == 64, "one digit value per lane of the tile's count column");

__global__ void __launch_bounds__(QRX_WG) quic_rx_select_kernel(const QuicRxArgs a, const QuicRxLimits lim)
{
    if (blockIdx.x == 0 && threadIdx.x < QRX_NSTATS)
        a.stats[threadIdx.x] = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * QRX_WG + threadIdx.x; k < a.n; k += (uint64_t)gridDim.x * QRX_WG) {
        const uint32_t type = a.info != nullptr ? a.info[k].type : 0u;
        a.scan.l0[k] = quic_rx_selectable(a.pkts[k], type, lim) ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(QRX_WG) quic_rx_compact_kernel(const QuicRxArgs a, const QuicRxLimits lim)
{
    for (uint64_t k = (uint64_t)blockIdx.x * QRX_WG + threadIdx.x; k < a.n; k += (uint64_t)gridDim.x * QRX_WG) {
        const ptls_hip_quic_packet_t p = a.pkts[k];
        const uint32_t type = a.info != nullptr ? a.info[k].type : 0u;
        if (!quic_rx_selectable(p, type, lim)) /* (the flag itself is gone: the scan wrote the prefix over it) */
            continue;
        const uint32_t at = scan_at(a.scan, k);
        a.sel[at] = (uint32_t)k;
        a.packed[at] = p;
        a.keys[at] = quic_rx_sort_key(p);
    }
}

__global__ void __launch_bounds__(QRX_WG) quic_rx_stats_kernel(const QuicRxArgs a)
{
    const uint32_t m = *a.total;
    uint64_t ghash = 0, blocks = 0, runs = 0;
    uint32_t max16 = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * QRX_WG + threadIdx.x; j < m; j += (uint64_t)gridDim.x * QRX_WG) {
        const ptls_hip_quic_packet_t p = a.packed[j];
        const uint32_t len = quic_rx_len(p);
        ghash += quic_rx_ghash_elems(p);
        blocks += len / 64u;
        if (j != 0 && a.packed[j - 1].key != p.key)
            ++runs;
        max16 = max(max16, len >> 4);
    }
    ghash = wave_sum(ghash);
    blocks = wave_sum(blocks);
    runs = wave_sum(runs);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        max16 = max(max16, (uint32_t)__shfl_xor((int)max16, d));
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(reinterpret_cast<unsigned long long *>(a.stats + QRX_STAT_GHASH), (unsigned long long)ghash);
        atomicAdd(reinterpret_cast<unsigned long long *>(a.stats + QRX_STAT_BLOCKS64), (unsigned long long)blocks);
        atomicAdd(reinterpret_cast<unsigned long long *>(a.stats + QRX_STAT_RUNS), (unsigned long long)runs);
        atomicMax(reinterpret_cast<unsigned long long *>(a.stats + QRX_STAT_MAX16), (unsigned long long)max16);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.stats[QRX_STAT_COUNT] = m;
        *a.chunk = Chunk{0u, m, 0xffffffffu, 0u};
    }
}

/* the digit of position t of a pass, or QRX_DIGITS past the end */
__device__ __forceinline__ uint32_t digit_at(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ src, uint32_t m,
                                             uint32_t shift, uint64_t t, uint32_t *v)
{
    if (t >= m)
        return QRX_DIGITS;
    *v = src != nullptr ? min(src[t], m - 1u) : (uint32_t)t; /* (a permutation of 0 .. m - 1: the bound holds a stray read inside) */
    return (keys[*v] >> shift) & (QRX_DIGITS - 1);
}

__global__ void __launch_bounds__(QRX_WG) quic_rx_hist_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ src,
                                                              uint32_t m, uint32_t shift, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t cnt[QRX_DIGITS];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, ntiles = gridDim.x;
    if (tid < QRX_DIGITS)
        cnt[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < QRX_ROUNDS; ++r) {
        uint32_t v;
        const uint32_t d = digit_at(keys, src, m, shift, (uint64_t)tile * QRX_TILE + (uint32_t)r * QRX_WG + tid, &v);
        if (d < QRX_DIGITS)
            atomicAdd(&cnt[d], 1u); /* (integer counts: any order of addition gives the same) */
    }
    __syncthreads();
    if (tid < QRX_DIGITS)
        hist[(uint64_t)tid * ntiles + tile] = cnt[tid];
}

__global__ void __launch_bounds__(QRX_WG) quic_rx_scatter_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ src,
                                                                 uint32_t m, uint32_t shift, const uint32_t *__restrict__ hl0,
                                                                 const uint32_t *__restrict__ hl1, const uint32_t *__restrict__ hl2,
                                                                 uint32_t *__restrict__ dst)
{
    __shared__ uint32_t cnt[QRX_WAVES][QRX_DIGITS]; /* per wave: positions of each digit in the rounds so far */
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, tile = blockIdx.x, ntiles = gridDim.x;
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
    cnt[wave][lane] = 0;
    __syncthreads();
    uint32_t v[QRX_ROUNDS], d[QRX_ROUNDS], rank[QRX_ROUNDS];
#pragma unroll
    for (int r = 0; r < QRX_ROUNDS; ++r) {
        /* wave w holds positions [256 w, 256 w + 256) of the tile, round r of them [64 r, 64 r + 64) */
        const uint64_t t = (uint64_t)tile * QRX_TILE + wave * (64u * QRX_ROUNDS) + (uint32_t)r * 64u + lane;
        v[r] = 0;
        d[r] = digit_at(keys, src, m, shift, t, &v[r]);
        /* the lanes of this round with my digit (a lane past the end matches no digit) */
        unsigned long long same = __ballot(d[r] < QRX_DIGITS);
#pragma unroll
        for (uint32_t b = 0; b < QRX_DIGIT_BITS; ++b) {
            const unsigned long long has = __ballot((d[r] >> b) & 1u);
            same &= ((d[r] >> b) & 1u) != 0 ? has : ~has;
        }
        const uint32_t before = (uint32_t)__popcll(same & below);
        const uint32_t dd = d[r] & (QRX_DIGITS - 1);
        rank[r] = cnt[wave][dd] + before;
        __syncthreads();
        if (d[r] < QRX_DIGITS && before == 0)
            cnt[wave][dd] += (uint32_t)__popcll(same);
        __syncthreads();
    }
    /* the global position of digit dd in this tile: the scanned [digit][tile] counts, then the waves in front of mine */
#pragma unroll
    for (int r = 0; r < QRX_ROUNDS; ++r) {
        if (d[r] >= QRX_DIGITS)
            continue;
        const uint64_t x = (uint64_t)d[r] * ntiles + tile;
        uint32_t at = hl0[x] + rank[r]; /* (scan_at written out: the three levels are this kernel's own __restrict__ pointers) */
        if (hl1 != nullptr)
            at += hl1[x / QP_SCAN_SPAN];
        if (hl2 != nullptr)
            at += hl2[x / ((uint64_t)QP_SCAN_SPAN * QP_SCAN_SPAN)];
#pragma unroll
        for (uint32_t w = 0; w + 1 < (uint32_t)QRX_WAVES; ++w)
            if (w < wave)
                at += cnt[w][d[r]];
        if (at < m)
            dst[at] = v[r];
    }
}

static unsigned entry_grid_check(unsigned grid)
{
    return grid != 0 ? grid : 1;
}

int launch_quic_rx_select(const QuicRxArgs &a, const QuicRxLimits &lim, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_rx_select_kernel, dim3(entry_grid_check(grid)), dim3(QRX_WG), 0, static_cast<hipStream_t>(stream), a, lim);
    return (int)hipGetLastError();
}

int launch_quic_rx_compact(const QuicRxArgs &a, const QuicRxLimits &lim, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_rx_compact_kernel, dim3(entry_grid_check(grid)), dim3(QRX_WG), 0, static_cast<hipStream_t>(stream), a, lim);
    return (int)hipGetLastError();
}

int launch_quic_rx_stats(const QuicRxArgs &a, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_rx_stats_kernel, dim3(entry_grid_check(grid)), dim3(QRX_WG), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

int launch_quic_rx_hist(const uint32_t *keys, const uint32_t *src, uint32_t m, uint32_t shift, uint32_t *hist, void *stream)
{
    const unsigned ntiles = (unsigned)(((uint64_t)m + QRX_TILE - 1) / QRX_TILE);
    hipLaunchKernelGGL(quic_rx_hist_kernel, dim3(entry_grid_check(ntiles)), dim3(QRX_WG), 0, static_cast<hipStream_t>(stream), keys, src, m,
                       shift, hist);
    return (int)hipGetLastError();
}

int launch_quic_rx_scatter(const uint32_t *keys, const uint32_t *src, uint32_t m, uint32_t shift, const uint32_t *hl0,
                           const uint32_t *hl1, const uint32_t *hl2, uint32_t *dst, void *stream)
{
    const unsigned ntiles = (unsigned)(((uint64_t)m + QRX_TILE - 1) / QRX_TILE);
    hipLaunchKernelGGL(quic_rx_scatter_kernel, dim3(entry_grid_check(ntiles)), dim3(QRX_WG), 0, static_cast<hipStream_t>(stream), keys, src,
                       m, shift, hl0, hl1, hl2, dst);
    return (int)hipGetLastError();
}

} // namespace ptls_hip
