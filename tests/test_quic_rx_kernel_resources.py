"""Resource guard of the device-side receive step's kernels, read from the built gfx950 code object
(hsig-picotls_amd/build/quic_rx_kernel.o, no GPU needed): exactly the five kernels of quic_rx_kernel.hip, none with a private
segment (the radix pass keeps its per-round values under compile-time indices; scratch would mean a runtime-indexed array or
a spill), and the LDS each was designed with: none for select, compact and the sums (wave shuffles, then integer atomics),
64 digit counts (256 bytes) for the histogram, 4 waves x 64 digit counts (1024 bytes) for the scatter."""
import os

import pytest

from test_quic_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "quic_rx_kernel.o")
LDS = {"quic_rx_select_kernel": 0, "quic_rx_compact_kernel": 0, "quic_rx_stats_kernel": 0, "quic_rx_hist_kernel": 256,
       "quic_rx_scatter_kernel": 1024}


@pytest.mark.skipif(not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="needs the in-tree build (__graft_entry__.build()) and the ROCm LLVM tools")
def test_quic_rx_kernels_have_no_scratch(tmp_path):
    ks = _kernels(OBJ, tmp_path)
    assert len(ks) == len(LDS), sorted(ks)
    for name, lds in LDS.items():
        mine = [k for k in ks if name in k]
        assert len(mine) == 1, (name, sorted(ks))
        assert ks[mine[0]] == (0, lds), (name, ks[mine[0]])
