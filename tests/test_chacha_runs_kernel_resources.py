"""Register-budget guard of the run-layout ChaCha20-Poly1305 kernel, read from the built gfx950 code object
(hsig-picotls_amd/build/chacha_runs_kernel.o, no GPU needed): it holds the 12 instantiations of chacha20poly1305_runs_kernel
(3 widths x seal / open x aligned / not) and none has a private segment (scratch).  The pieces, the keystream block and the
Poly1305 state live in named registers through both transposes; scratch would mean a spill or a runtime-indexed array."""
import os

import pytest

from test_chacha_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "chacha_runs_kernel.o")


@pytest.mark.skipif(not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="needs the in-tree build (__graft_entry__.build()) and the ROCm LLVM tools")
def test_chacha_runs_kernels_have_no_scratch(tmp_path):
    ks = _kernels(OBJ, tmp_path)
    runs = [k for k in ks if "chacha20poly1305_runs_kernel" in k]
    assert len(runs) == 12 and len(ks) == 12, sorted(ks)
    assert all(ks[k] == 0 for k in runs), {k: ks[k] for k in runs if ks[k]}
