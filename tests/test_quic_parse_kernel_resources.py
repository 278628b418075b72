"""Resource guard of the datagram-parsing kernels, read from the built gfx950 code object
(hsig-picotls_amd/build/quic_parse_kernel.o, no GPU needed): none of the three kernels has a private segment (the walk state
is scalars, the CID compare reads the packet and the table entry directly; scratch would mean a runtime-indexed array or a
spill), the two walk kernels use no LDS, and the scan kernel holds its 256 thread sums, 1024 bytes."""
import os

import pytest

from test_quic_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "quic_parse_kernel.o")


@pytest.mark.skipif(not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="needs the in-tree build (__graft_entry__.build()) and the ROCm LLVM tools")
def test_quic_parse_kernels_have_no_scratch(tmp_path):
    ks = _kernels(OBJ, tmp_path)
    count = [k for k in ks if "quic_parse_count_kernel" in k]
    scan = [k for k in ks if "quic_parse_scan_kernel" in k]
    write = [k for k in ks if "quic_parse_write_kernel" in k]
    assert len(count) == 1 and len(scan) == 1 and len(write) == 1 and len(ks) == 3, sorted(ks)
    assert all(ks[k][0] == 0 for k in ks), ks
    assert ks[count[0]][1] == 0 and ks[write[0]][1] == 0 and ks[scan[0]][1] == 1024, ks
