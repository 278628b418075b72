"""Resource guard of the ACK-frame kernels, read from the built gfx950 code object (hsig-picotls_amd/build/quic_ack_kernel.o,
no GPU needed): exactly the two kernels of quic_ack_kernel.hip, none with a private segment and none with LDS: a frame is never
built in a byte array in registers (indexed at run time, that would become a private segment); every field goes to global
memory as it is produced, and the offsets come from the scan levels of quic_parse_kernel.hip."""
import os

import pytest

from test_quic_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "quic_ack_kernel.o")


@pytest.mark.skipif(not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="needs the in-tree build (__graft_entry__.build()) and the ROCm LLVM tools")
def test_quic_ack_kernels_have_no_scratch_and_no_lds(tmp_path):
    ks = _kernels(OBJ, tmp_path)
    size = [k for k in ks if "quic_ack_size_kernel" in k]
    write = [k for k in ks if "quic_ack_write_kernel" in k]
    assert len(size) == 1 and len(write) == 1 and len(ks) == 2, sorted(ks)
    assert all(ks[k][0] == 0 for k in ks), ks
    assert all(ks[k][1] == 0 for k in ks), ks
