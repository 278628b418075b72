/*
 * quic_ack_kernel.hip -- ACK frames written on the device from the tracked packet numbers, and the send requests that carry
 * them (include/ptls_hip.h 2m).  The rule is quic_ack.h's.
 *
 *   quic_ack_size_kernel   a thread per list entry: the status from the entry's state, the frame length (two varint lengths
 *                          and a population count of run starts) into the length levels, the flag "has a frame" into the flag
 *                          levels
 *   quic_ack_write_kernel  a thread per list entry, behind the scan levels of quic_parse_kernel.hip over both: the three
 *                          per-entry outputs, the frame stored field by field at its offset (the runs walked with
 *                          count-trailing-zeros on the window and its complement), the request at the compacted position.  The
 *                          thread of the last list entry holds both totals (its prefixes plus its own terms) and stores them:
 *                          no atomic, and nothing to reset between calls
 *
 * The state table is read and never written.  Every loop is a grid stride, or bounded by 31 runs or 8 varint bytes.  No kernel
 * has a private segment or uses LDS: no byte array is built in registers, every field goes straight to global memory.
 */
#include <hip/hip_runtime.h>

#include "internal.h"
#include "quic_scan.h"
#include "quic_ack.h"

namespace ptls_hip {

constexpr int QAK_WG = 256;

__global__ void __launch_bounds__(QAK_WG) quic_ack_size_kernel(const QuicAckArgs a)
{
    for (uint64_t j = (uint64_t)blockIdx.x * QAK_WG + threadIdx.x; j < a.n; j += (uint64_t)gridDim.x * QAK_WG) {
        ptls_hip_quic_pnspace_t st;
        uint32_t len;
        (void)quic_ack_judge(a.spaces, a.count, a.space, a.list[j], a.ack_delay, a.max_ranges, &st, &len);
        a.lens.l0[j] = len;
        a.flags.l0[j] = len != 0 ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(QAK_WG) quic_ack_write_kernel(const QuicAckArgs a)
{
    for (uint64_t j = (uint64_t)blockIdx.x * QAK_WG + threadIdx.x; j < a.n; j += (uint64_t)gridDim.x * QAK_WG) {
        const uint32_t conn = a.list[j];
        ptls_hip_quic_pnspace_t st;
        uint32_t len;
        const uint32_t status = quic_ack_judge(a.spaces, a.count, a.space, conn, a.ack_delay, a.max_ranges, &st, &len);
        const uint32_t off = scan_at(a.lens, j), pos = scan_at(a.flags, j); /* (the scans wrote the prefixes over the terms) */
        a.status[j] = status;
        a.frame_off[j] = off;
        a.frame_len[j] = len;
        if (status == PTLS_HIP_QUIC_ACK_OK) {
            (void)quic_ack_write(a.frames + off, st.next, st.window, a.ack_delay, a.max_ranges);
            a.reqs[pos] = quic_ack_request(a.in_off, off, a.pkt_base, a.pkt_stride, pos, conn, len);
        }
        if (j == (uint64_t)a.n - 1) {
            a.sums[0] = (uint64_t)off + len;
            a.sums[1] = (uint64_t)pos + (len != 0 ? 1u : 0u);
        }
    }
}

int launch_quic_ack_size(const QuicAckArgs &a, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_ack_size_kernel, dim3(grid != 0 ? grid : 1), dim3(QAK_WG), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

int launch_quic_ack_write(const QuicAckArgs &a, unsigned grid, void *stream)
{
    hipLaunchKernelGGL(quic_ack_write_kernel, dim3(grid != 0 ? grid : 1), dim3(QAK_WG), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

} // namespace ptls_hip
