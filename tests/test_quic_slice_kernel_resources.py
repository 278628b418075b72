"""Resource guard of the copy transport's QUIC header-return kernel, read from the built gfx950 code object
(hsig-picotls_amd/build/quic_slice_kernel.o, no GPU needed) the way tests/test_quic_kernel_resources.py reads
quic_kernel.o: quic_pack_headers_kernel is the object's only kernel and has neither a private segment (scratch: the header
bytes are selected under compile-time indices) nor LDS."""
import os

import pytest

from test_quic_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "quic_slice_kernel.o")


@pytest.mark.skipif(not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="needs the in-tree build (__graft_entry__.build()) and the ROCm LLVM tools")
def test_quic_slice_kernel_has_no_scratch_and_no_lds(tmp_path):
    ks = _kernels(OBJ, tmp_path)
    assert len(ks) == 1 and "quic_pack_headers_kernel" in next(iter(ks)), sorted(ks)
    assert all(v == (0, 0) for v in ks.values()), ks
