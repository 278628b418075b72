"""CPU tests of the ChaCha20-Poly1305 host-pipeline surface of libptls_hip.so: the library exports the new entry points, the
binding declares them, and NULL or bad arguments fail with PTLS_HIP_EINVAL or NULL before any device call."""
import ctypes
import os
import re

import ptls_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("ptls_hip_pipeline_new_algo", "ptls_hip_pipeline_algo", "ptls_hip_pipeline_set_chacha_lanes")


def test_library_exports_the_pipeline_symbols():
    L = ptls_hip.lib()
    for name in FUNCTIONS:
        assert hasattr(L, name), name
        assert name in ptls_hip.SIGNATURES, name
    assert (ptls_hip.CHACHA_LAYOUT_AUTO, ptls_hip.CHACHA_LAYOUT_BLOCKS, ptls_hip.CHACHA_LAYOUT_RUNS) == (0, 1, 2)
    # the binding's constants are the header's
    src = open(os.path.join(ROOT, "include", "ptls_hip.h")).read()
    for name in ("AUTO", "BLOCKS", "RUNS"):
        m = re.search(r"#define PTLS_HIP_CHACHA_LAYOUT_%s (\d+)" % name, src)
        assert m and int(m.group(1)) == getattr(ptls_hip, "CHACHA_LAYOUT_" + name)


def test_pipeline_new_algo_argument_checks():
    """a NULL engine, an unknown algorithm or a slice below 64 KiB: NULL and a message; a non-NULL engine pointer is not
    dereferenced before the other arguments pass, so this runs without a GPU"""
    L = ptls_hip.lib()
    for algo in (ptls_hip.ALGO_AESGCM, ptls_hip.ALGO_CHACHA20POLY1305, 0, 3):
        assert L.ptls_hip_pipeline_new_algo(None, algo, 1 << 20) is None
        assert "bad arguments" in ptls_hip.last_error()
    fake = ctypes.create_string_buffer(256)
    for algo, slice_bytes in ((0, 1 << 20), (3, 1 << 20), (-1, 1 << 20), (ptls_hip.ALGO_CHACHA20POLY1305, (1 << 16) - 1),
                              (ptls_hip.ALGO_AESGCM, 0)):
        assert L.ptls_hip_pipeline_new_algo(ctypes.addressof(fake), algo, slice_bytes) is None
        assert "pipeline_new: bad arguments" in ptls_hip.last_error()
    assert L.ptls_hip_pipeline_new(None, 1 << 20) is None  # the AES-GCM constructor goes the same way


def test_null_pipeline_is_refused():
    L = ptls_hip.lib()
    assert L.ptls_hip_pipeline_algo(None) == ptls_hip.EINVAL
    for lanes, layout in ((0, 0), (4, ptls_hip.CHACHA_LAYOUT_RUNS), (3, 7)):
        assert L.ptls_hip_pipeline_set_chacha_lanes(None, lanes, layout) == ptls_hip.EINVAL
        assert "pipeline_set_chacha_lanes" in ptls_hip.last_error()
