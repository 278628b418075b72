"""Register-budget guard of the ChaCha20-Poly1305 kernels, read from the built gfx950 code object
(hsig-picotls_amd/build/chacha_kernel.o, no GPU needed): no instantiation of chacha20poly1305_batch_kernel and no mask kernel
has a private segment (scratch).  Their whole state (the ChaCha block, the Poly1305 accumulator and the record's powers of r)
is meant to live in named registers; scratch would mean a runtime-indexed array or a spill, streamed out to HBM per record."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "hsig-picotls_amd", "build")
LLVM = "/opt/rocm/lib/llvm/bin"


def _kernels(obj, tmp_path):
    """{kernel symbol: private_segment_fixed_size} of the gfx950 code object bundled into a host object"""
    fat, co = tmp_path / "fat.bin", tmp_path / "k.co"
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, str(fat)], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.private_segment_fixed_size:\s+(\d+)", line)
        if m and name is not None:
            out[name] = int(m.group(1))
    return out


@pytest.mark.skipif(not os.path.exists(os.path.join(BUILD, "chacha_kernel.o")) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="needs the in-tree build (__graft_entry__.build()) and the ROCm LLVM tools")
def test_chacha_kernels_have_no_scratch(tmp_path):
    ks = _kernels(os.path.join(BUILD, "chacha_kernel.o"), tmp_path)
    batch = [k for k in ks if "chacha20poly1305_batch_kernel" in k]
    mask = [k for k in ks if "chacha20_mask_kernel" in k]
    assert len(batch) == 16 and len(mask) == 1, sorted(ks)  # 4 widths x seal / open x aligned / not
    assert all(ks[k] == 0 for k in batch + mask), {k: ks[k] for k in batch + mask if ks[k]}
    assert all(v == 0 for v in ks.values()), ks  # the key set-up kernel as well
