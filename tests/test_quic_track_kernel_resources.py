"""Resource guard of the packet-number tracking kernels, read from the built gfx950 code object
(hsig-picotls_amd/build/quic_track_kernel.o, no GPU needed): exactly the three kernels of quic_track_kernel.hip, none with a
private segment and none with LDS: the table, the maxima and the window bits go through integer atomics in device memory, the
positions of the touched list through the scan levels of quic_parse_kernel.hip."""
import os

import pytest

from test_quic_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "quic_track_kernel.o")


@pytest.mark.skipif(not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="needs the in-tree build (__graft_entry__.build()) and the ROCm LLVM tools")
def test_quic_track_kernels_have_no_scratch_and_no_lds(tmp_path):
    ks = _kernels(OBJ, tmp_path)
    claim = [k for k in ks if "quic_track_claim_kernel" in k]
    verdict = [k for k in ks if "quic_track_verdict_kernel" in k]
    apply_ = [k for k in ks if "quic_track_apply_kernel" in k]
    assert len(claim) == 1 and len(verdict) == 1 and len(apply_) == 1 and len(ks) == 3, sorted(ks)
    assert all(ks[k][0] == 0 for k in ks), ks
    assert all(ks[k][1] == 0 for k in ks), ks
