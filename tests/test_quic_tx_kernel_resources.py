"""Resource guard of the send object's kernels, read from the built gfx950 code object
(hsig-picotls_amd/build/quic_tx_kernel.o, no GPU needed): exactly the six kernels of quic_tx_kernel.hip, none with a private
segment and none with LDS: the first run of a connection goes through an integer atomic in device memory, the run indices and
the compacted positions through the scan levels of quic_parse_kernel.hip, the plan order through the radix passes of
quic_rx_kernel.hip."""
import os

import pytest

from test_quic_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "quic_tx_kernel.o")
NAMES = ("quic_tx_heads_kernel", "quic_tx_runs_kernel", "quic_tx_select_kernel", "quic_tx_build_kernel", "quic_tx_apply_kernel",
         "quic_tx_order_kernel")


@pytest.mark.skipif(not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="needs the in-tree build (__graft_entry__.build()) and the ROCm LLVM tools")
def test_quic_tx_kernels_have_no_scratch_and_no_lds(tmp_path):
    ks = _kernels(OBJ, tmp_path)
    for name in NAMES:
        assert len([k for k in ks if name in k]) == 1, (name, sorted(ks))
    assert len(ks) == len(NAMES), sorted(ks)
    assert all(ks[k][0] == 0 for k in ks), ks
    assert all(ks[k][1] == 0 for k in ks), ks
