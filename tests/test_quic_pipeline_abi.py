"""CPU tests of the QUIC host-pipeline surface of libptls_hip.so (include/ptls_hip.h 2g): the library exports the two entry
points, the binding declares them, and a null pipeline, keyset or buffer fails with PTLS_HIP_EINVAL and a message before
anything is dereferenced (the non-null objects here are zeroed memory, not pipelines or keysets), so this runs without a
GPU."""
import ctypes
import os
import re

import numpy as np

import ptls_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("ptls_hip_pipeline_quic_seal", "ptls_hip_pipeline_quic_open")


def test_library_exports_the_quic_pipeline_symbols():
    L = ptls_hip.lib()
    src = open(os.path.join(ROOT, "include", "ptls_hip.h")).read()
    for name in FUNCTIONS:
        assert hasattr(L, name), name
        assert name in ptls_hip.SIGNATURES, name
        assert re.search(r"\bint %s\(" % name, src), name
    assert len(ptls_hip.SIGNATURES["ptls_hip_pipeline_quic_seal"][1]) == 7
    assert len(ptls_hip.SIGNATURES["ptls_hip_pipeline_quic_open"][1]) == 9
    assert callable(ptls_hip.Pipeline.quic_seal) and callable(ptls_hip.Pipeline.quic_open)


def _args():
    fake = [ctypes.create_string_buffer(512) for _ in range(3)]
    pkts = np.zeros(2, dtype=ptls_hip.QUIC_PACKET_DTYPE)
    bufs = [np.zeros(64, np.uint8) for _ in range(4)]
    return fake, pkts, bufs


def test_null_objects_are_refused():
    L = ptls_hip.lib()
    fake, pkts, b = _args()
    p, ks, hp = (ctypes.addressof(x) for x in fake)
    pk, b0, b1, b2, b3 = pkts.ctypes.data, *(x.ctypes.data for x in b)
    for n in (0, 2):
        for args in ((None, ks, hp), (p, None, hp), (p, ks, None), (None, None, None)):
            assert L.ptls_hip_pipeline_quic_seal(*args, pk, n, b0, b1) == ptls_hip.EINVAL
            assert "pipeline_quic_seal: null pipeline or keyset" in ptls_hip.last_error()
            assert L.ptls_hip_pipeline_quic_open(*args, pk, n, b0, b1, b2, b3) == ptls_hip.EINVAL
            assert "pipeline_quic_open: null pipeline or keyset" in ptls_hip.last_error()
    assert all(not x.any() for x in b)


def test_null_buffers_are_refused():
    """with n != 0, before the (fake) pipeline and keysets are looked at"""
    L = ptls_hip.lib()
    fake, pkts, b = _args()
    p, ks, hp = (ctypes.addressof(x) for x in fake)
    pk, b0, b1, b2, b3 = pkts.ctypes.data, *(x.ctypes.data for x in b)
    for args in ((None, b0, b1), (pk, None, b1), (pk, b0, None)):
        assert L.ptls_hip_pipeline_quic_seal(p, ks, hp, args[0], 2, *args[1:]) == ptls_hip.EINVAL
        assert "pipeline_quic_seal: null buffer" in ptls_hip.last_error()
    for args in ((None, b0, b1, b2, b3), (pk, None, b1, b2, b3), (pk, b0, None, b2, b3), (pk, b0, b1, None, b3), (pk, b0, b1, b2, None)):
        assert L.ptls_hip_pipeline_quic_open(p, ks, hp, args[0], 2, *args[1:]) == ptls_hip.EINVAL
        assert "pipeline_quic_open: null buffer" in ptls_hip.last_error()
    assert all(not x.any() for x in b)
