"""Resource guard of the QUIC header-protection kernels, read from the built gfx950 code object
(hsig-picotls_amd/build/quic_kernel.o, no GPU needed): neither quic_protect_kernel nor any instantiation of
quic_unprotect_kernel (AES-128, AES-256, ChaCha20) has a private segment (scratch).  The mask travels as two words and the
header bytes are handled under compile-time indices; scratch would mean a runtime-indexed array or a spill.  The ChaCha20
instantiation uses no LDS; the AES ones hold the replicated T-tables of aesecb_batch_kernel."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "hsig-picotls_amd", "build")
LLVM = "/opt/rocm/lib/llvm/bin"


def _kernels(obj, tmp_path):
    """{kernel symbol: (private_segment_fixed_size, group_segment_fixed_size)} of the gfx950 code object of a host object"""
    fat, co = tmp_path / "fat.bin", tmp_path / "k.co"
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, str(fat)], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    out, cur = {}, {}
    for line in notes.splitlines():
        for field in ("name", "private_segment_fixed_size", "group_segment_fixed_size"):
            m = re.match(r"\s+(?:- )?\.%s:\s+(\S+)" % field, line)
            if m:
                cur[field] = m.group(1)
        if len(cur) == 3:
            out[cur["name"]] = (int(cur["private_segment_fixed_size"]), int(cur["group_segment_fixed_size"]))
            cur = {}
    return out


@pytest.mark.skipif(not os.path.exists(os.path.join(BUILD, "quic_kernel.o")) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="needs the in-tree build (__graft_entry__.build()) and the ROCm LLVM tools")
def test_quic_kernels_have_no_scratch(tmp_path):
    ks = _kernels(os.path.join(BUILD, "quic_kernel.o"), tmp_path)
    unprotect = [k for k in ks if "quic_unprotect_kernel" in k]
    protect = [k for k in ks if "quic_protect_kernel" in k]
    assert len(unprotect) == 3 and len(protect) == 1 and len(ks) == 4, sorted(ks)
    assert all(ks[k][0] == 0 for k in ks), ks
    lds = sorted(ks[k][1] for k in unprotect)
    assert lds == [0, 131072, 131072] and ks[protect[0]][1] == 0, ks
