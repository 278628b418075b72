"""CPU tests of the packet-number tracking surface (include/ptls_hip.h 2k): the library exports the entry points and the
binding declares them with the header's signatures, the two structs' layouts and the verdict constants match the header, and
every refusal that can be reached without a device fails with its message and launches nothing.  The refusals that need an
open call in front of them live in tests/test_gpu_quic_track.py."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import ptls_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("ptls_hip_quic_rx_track", "ptls_hip_quic_rx_track_timing")


def _header():
    with open(os.path.join(ROOT, "include", "ptls_hip.h")) as f:
        return f.read()


def test_library_exports_the_track_symbols():
    L = ptls_hip.lib()
    header = _header()
    for name in FUNCTIONS:
        assert hasattr(L, name), name
        assert name in ptls_hip.SIGNATURES, name
    # the binding's argument lists against the header's declarations
    decl = re.search(r"int ptls_hip_quic_rx_track\(([^;]*)\);", header).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["rx", "tr", "d_sel", "d_result", "d_pn_out", "n_touched", "stream"]
    res, args = ptls_hip.SIGNATURES["ptls_hip_quic_rx_track"]
    assert res is ctypes.c_int and len(args) == 7 and args[5] is ctypes.POINTER(ctypes.c_size_t)
    assert "void ptls_hip_quic_rx_track_timing(float *track_ms);" in header
    assert ptls_hip.SIGNATURES["ptls_hip_quic_rx_track_timing"] == (None, [ctypes.POINTER(ctypes.c_float)])
    for name, value in (("NONE", 0), ("NEW", 1), ("DUPLICATE", 2), ("TOO_OLD", 3)):
        assert re.search(r"#define PTLS_HIP_QUIC_PN_%s %du\b" % (name, value), header), name
        assert getattr(ptls_hip, "QUIC_PN_" + name) == value


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptls_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu\\n", sizeof(ptls_hip_quic_pnspace_t), offsetof(ptls_hip_quic_pnspace_t, next),\n'
                   '           offsetof(ptls_hip_quic_pnspace_t, window));\n'
                   '    printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ptls_hip_quic_rx_track_t), offsetof(ptls_hip_quic_rx_track_t, d_spaces),\n'
                   '           offsetof(ptls_hip_quic_rx_track_t, count), offsetof(ptls_hip_quic_rx_track_t, d_expected_pn),\n'
                   '           offsetof(ptls_hip_quic_rx_track_t, expected_count), offsetof(ptls_hip_quic_rx_track_t, d_verdict),\n'
                   '           offsetof(ptls_hip_quic_rx_track_t, d_touched));\n'
                   '    printf("%u %u %u %u\\n", PTLS_HIP_QUIC_PN_NONE, PTLS_HIP_QUIC_PN_NEW, PTLS_HIP_QUIC_PN_DUPLICATE, PTLS_HIP_QUIC_PN_TOO_OLD);\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = ptls_hip.QUIC_PNSPACE_DTYPE
    assert out[:3] == [D.itemsize, D.fields["next"][1], D.fields["window"][1]] == [16, 0, 8]
    T = ptls_hip.QuicRxTrack
    assert out[3:10] == [ctypes.sizeof(T), T.d_spaces.offset, T.count.offset, T.d_expected_pn.offset, T.expected_count.offset,
                         T.d_verdict.offset, T.d_touched.offset] == [48, 0, 8, 16, 24, 32, 40]
    assert out[10:] == [ptls_hip.QUIC_PN_NONE, ptls_hip.QUIC_PN_NEW, ptls_hip.QUIC_PN_DUPLICATE, ptls_hip.QUIC_PN_TOO_OLD]


def test_refusals_without_a_device():
    L = ptls_hip.lib()
    fake = ctypes.create_string_buffer(256)  # an "engine": never dereferenced before the checks pass
    rx = L.ptls_hip_quic_rx_new(ctypes.addressof(fake), 0, 4)
    assert rx
    buf = 0x1000  # a "device" address: never read by the host
    try:
        n = ctypes.c_size_t(77)

        def track(obj=rx, tr=(buf, 8, buf, 24, buf, buf), sel=buf, res=buf, pn=buf, n_touched=n):
            s = ptls_hip.QuicRxTrack(*tr) if tr is not None else None
            return L.ptls_hip_quic_rx_track(obj, ctypes.addressof(s) if s is not None else None, sel, res, pn,
                                            ctypes.byref(n_touched) if n_touched is not None else None, None)

        for kw in (dict(obj=None), dict(tr=None), dict(sel=None), dict(res=None), dict(pn=None), dict(n_touched=None)):
            assert track(**kw) == ptls_hip.EINVAL, kw
            assert "quic_rx_track: null receive object, parameters, array or n_touched" in ptls_hip.last_error(), kw
        for tr in ((None, 8, buf, 24, buf, buf), (buf, 8, buf, 24, None, buf), (buf, 8, buf, 24, buf, None)):
            assert track(tr=tr) == ptls_hip.EINVAL, tr
            assert "quic_rx_track: null state, verdict or touched array" in ptls_hip.last_error(), tr
        for count in (0, 1 << 32):
            assert track(tr=(buf, count, buf, 24, buf, buf)) == ptls_hip.EINVAL
            assert "quic_rx_track: a connection count of %d is outside 1 .. 2^32 - 1" % count in ptls_hip.last_error()
        assert track(tr=(buf, 8, None, 24, buf, buf)) == ptls_hip.EINVAL
        assert "quic_rx_track: no expected-pn table, but 24 entries of it" in ptls_hip.last_error()
        for tr in ((buf, 8, buf, 24, buf, buf), (buf, 8, None, 0, buf, buf)):  # well-formed, but nothing was opened
            assert track(tr=tr) == ptls_hip.EINVAL
            assert "quic_rx_track: no open call on the object since its entries were loaded" in ptls_hip.last_error()
        assert n.value == 77  # nothing written by a refused call
        L.ptls_hip_quic_rx_track_timing(None)  # no output asked for: a no-op
        ms = ctypes.c_float(-1)
        L.ptls_hip_quic_rx_track_timing(ctypes.byref(ms))
        assert ms.value == 0  # nothing was timed on this thread
    finally:
        L.ptls_hip_quic_rx_free(rx)
