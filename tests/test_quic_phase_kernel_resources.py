"""Resource guard of the key-phase kernels, read from the built gfx950 code object
(hsig-picotls_amd/build/quic_phase_kernel.o, no GPU needed): exactly the five kernels of quic_phase_kernel.hip, none with a
private segment.  The three instantiations of quic_unprotect_phase_kernel share quic_unprotect_kernel's body and keep its LDS
(none for ChaCha20, the replicated AES T-tables otherwise); the two commit kernels use none: the minima go through 64-bit
integer atomics in device memory, the positions through the scan levels of quic_parse_kernel.hip."""
import os

import pytest

from test_quic_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "quic_phase_kernel.o")


@pytest.mark.skipif(not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="needs the in-tree build (__graft_entry__.build()) and the ROCm LLVM tools")
def test_quic_phase_kernels_have_no_scratch(tmp_path):
    ks = _kernels(OBJ, tmp_path)
    header = [k for k in ks if "quic_unprotect_phase_kernel" in k]
    mark = [k for k in ks if "quic_phase_mark_kernel" in k]
    apply_ = [k for k in ks if "quic_phase_apply_kernel" in k]
    assert len(header) == 3 and len(mark) == 1 and len(apply_) == 1 and len(ks) == 5, sorted(ks)
    assert all(ks[k][0] == 0 for k in ks), ks
    assert sorted(ks[k][1] for k in header) == [0, 131072, 131072], ks
    assert ks[mark[0]][1] == 0 and ks[apply_[0]][1] == 0, ks
