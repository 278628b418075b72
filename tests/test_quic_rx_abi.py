"""CPU tests of the receive object's surface (include/ptls_hip.h 2i): the library exports the entry points and the binding
declares them, the report's layout matches the header, and every refusal that can be reached without a device fails with its
message and launches nothing: the engine pointer is never dereferenced (a receive object allocates device memory with the
first use of each array) and the "keysets" are never read before the checks in front of them pass.  The refusals that
compare real keysets (engines, algorithms, key sizes) and the overlap check live in tests/test_gpu_quic_rx.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptls_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("ptls_hip_quic_rx_new", "ptls_hip_quic_rx_free", "ptls_hip_quic_rx_parse", "ptls_hip_quic_rx_set_packets",
             "ptls_hip_quic_rx_packets", "ptls_hip_quic_rx_info", "ptls_hip_quic_rx_count", "ptls_hip_quic_rx_open",
             "ptls_hip_quic_rx_set_plan", "ptls_hip_quic_rx_order", "ptls_hip_quic_rx_timing")


def test_library_exports_the_rx_symbols():
    L = ptls_hip.lib()
    with open(os.path.join(ROOT, "include", "ptls_hip.h")) as f:
        header = f.read()
    for name in FUNCTIONS:
        assert hasattr(L, name), name
        assert name in ptls_hip.SIGNATURES, name
        assert name + "(" in header, name
    assert len(ptls_hip.SIGNATURES["ptls_hip_quic_rx_open"][1]) == 13
    assert len(ptls_hip.SIGNATURES["ptls_hip_quic_rx_parse"][1]) == 9


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_report_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptls_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu\\n", sizeof(ptls_hip_quic_rx_report_t), offsetof(ptls_hip_quic_rx_report_t, n_selected),\n'
                   '           offsetof(ptls_hip_quic_rx_report_t, planned_on_device), offsetof(ptls_hip_quic_rx_report_t, lanes));\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    R = ptls_hip.QuicRxReport
    assert [int(x) for x in out] == [ctypes.sizeof(R), R.n_selected.offset, R.planned_on_device.offset, R.lanes.offset] == [16, 0, 8, 12]


def _fake():
    return ctypes.create_string_buffer(256)  # never dereferenced before the checks pass


def test_rx_new_refusals_and_null_objects():
    L = ptls_hip.lib()
    fake = _fake()
    eng = ctypes.addressof(fake)
    assert L.ptls_hip_quic_rx_new(None, 4, 4) is None and "quic_rx_new: null engine" in ptls_hip.last_error()
    assert L.ptls_hip_quic_rx_new(eng, 4, 0) is None and "cap 0 outside" in ptls_hip.last_error()
    assert L.ptls_hip_quic_rx_new(eng, 4, 1 << 32) is None and "quic_rx_new" in ptls_hip.last_error()
    assert L.ptls_hip_quic_rx_new(eng, 1 << 32, 4) is None and "max_dgrams 4294967296" in ptls_hip.last_error()
    L.ptls_hip_quic_rx_free(None)  # a no-op
    assert L.ptls_hip_quic_rx_packets(None) is None and L.ptls_hip_quic_rx_info(None) is None
    assert L.ptls_hip_quic_rx_order(None) is None and L.ptls_hip_quic_rx_count(None) == 0
    assert L.ptls_hip_quic_rx_set_plan(None, 0) == ptls_hip.EINVAL and "quic_rx_set_plan" in ptls_hip.last_error()
    rx = L.ptls_hip_quic_rx_new(eng, 0, 1)  # no datagrams ever: only rx_set_packets loads it
    assert rx
    L.ptls_hip_quic_rx_free(rx)  # nothing was allocated: no device is touched


def test_refusals_without_a_device():
    L = ptls_hip.lib()
    fake, ks, hp = _fake(), _fake(), _fake()
    eng = ctypes.addressof(fake)
    rx = L.ptls_hip_quic_rx_new(eng, 3, 4)
    assert rx
    try:
        # the plan mode
        for mode in (-1, 3, 64):
            assert L.ptls_hip_quic_rx_set_plan(rx, mode) == ptls_hip.EINVAL and "a mode other than 0" in ptls_hip.last_error()
        for mode in (1, 2, 0):
            assert L.ptls_hip_quic_rx_set_plan(rx, mode) == 0
        # rx_parse: 2h's refusals under this call's name, and the object's own limits
        dg = np.zeros(4, dtype=ptls_hip.QUIC_DATAGRAM_DTYPE)
        dg["off"], dg["len"] = (0, 100, 200, 300), (100, 100, 56, 10)
        n_pkts = ctypes.c_size_t(77)
        buf = 0x1000  # a "device" address: never read by the host

        def parse(obj=rx, params=None, dgrams=dg, n=3, d_buf=buf, buf_len=256, out=n_pkts, cmap=None):
            p = params if params is not None else ptls_hip.QuicParseParams(8, 16, 1, 0, None, 0)
            return L.ptls_hip_quic_rx_parse(obj, ctypes.addressof(p) if p is not False else None, cmap,
                                            dgrams.ctypes.data if dgrams is not None else None, n, d_buf, buf_len,
                                            ctypes.byref(out) if out is not None else None, None)

        for kw, msg in ((dict(obj=None), "null receive object"), (dict(params=False), "null receive object, parameters"),
                        (dict(out=None), "n_pkts"), (dict(dgrams=None), "null datagram array or buffer"),
                        (dict(d_buf=None), "null datagram array or buffer"),
                        (dict(n=4, buf_len=1024), "4 datagrams, the receive object was made for 3"),
                        (dict(params=ptls_hip.QuicParseParams(21, 16, 1, 0, None, 0)), "short_cid_len 21 is above 20"),
                        (dict(params=ptls_hip.QuicParseParams(8, 0, 1, 0, None, 0)), "max_per_dgram 0 is outside 1..16"),
                        (dict(params=ptls_hip.QuicParseParams(8, 17, 1, 0, None, 0)), "max_per_dgram 17 is outside 1..16"),
                        (dict(params=ptls_hip.QuicParseParams(8, 16, 1, 1, None, 0)), "reserved must be 0"),
                        (dict(buf_len=255), "datagram 2: off 200 + len 56 is past the buffer of 255 bytes")):
            assert parse(**kw) == ptls_hip.EINVAL, kw
            assert "quic_rx_parse:" in ptls_hip.last_error() and msg in ptls_hip.last_error(), (kw, ptls_hip.last_error())
        big = dg.copy()
        big["len"][1] = 65536
        assert parse(dgrams=big, buf_len=1 << 20) == ptls_hip.EINVAL and "datagram 1: len 65536 is above 65535" in ptls_hip.last_error()
        other = _fake()
        m = L.ptls_hip_quic_cidmap_new(ctypes.addressof(other), 4)
        try:
            assert parse(cmap=m) == ptls_hip.EINVAL and "belongs to another engine" in ptls_hip.last_error()
        finally:
            L.ptls_hip_quic_cidmap_free(m)
        assert n_pkts.value == 77 and L.ptls_hip_quic_rx_count(rx) == 0
        assert parse(n=0, dgrams=None, d_buf=None) == 0 and n_pkts.value == 0  # no datagrams: no device needed
        # rx_set_packets
        assert L.ptls_hip_quic_rx_set_packets(None, buf, None, 1, None) == ptls_hip.EINVAL
        assert "quic_rx_set_packets: null receive object" in ptls_hip.last_error()
        assert L.ptls_hip_quic_rx_set_packets(rx, None, None, 1, None) == ptls_hip.EINVAL
        assert L.ptls_hip_quic_rx_set_packets(rx, buf, None, 5, None) == ptls_hip.EINVAL
        assert "5 descriptors, the receive object holds 4" in ptls_hip.last_error()
        assert L.ptls_hip_quic_rx_set_packets(rx, None, None, 0, None) == 0
        assert L.ptls_hip_quic_rx_count(rx) == 0 and L.ptls_hip_quic_rx_packets(rx) is None and L.ptls_hip_quic_rx_order(rx) is None
        # rx_open: the null arguments (the keysets behind them are never read)
        rep = ptls_hip.QuicRxReport(5, 5, 5)
        k, h, r = ctypes.addressof(ks), ctypes.addressof(hp), ctypes.addressof(rep)
        for args in ((None, k, h, r), (rx, None, h, r), (rx, k, None, r), (rx, k, h, None)):
            assert L.ptls_hip_quic_rx_open(args[0], args[1], args[2], 0xFF, buf, 16, buf + 64, 16, buf, buf, buf, args[3],
                                           None) == ptls_hip.EINVAL
            assert "quic_rx_open: null receive object, keyset or report" in ptls_hip.last_error()
        assert (rep.n_selected, rep.planned_on_device, rep.lanes) == (5, 5, 5)  # nothing written by a refused call
    finally:
        L.ptls_hip_quic_rx_free(rx)
