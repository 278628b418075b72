"""CPU tests of the ACK-frame call's surface (include/ptls_hip.h 2m): the library exports the entry points and the binding
declares them with the header's signatures, the structs' layouts and the constants match the header, and every refusal fails
with its message, launches nothing and writes nothing: none of them needs a device."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import ptls_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("ptls_hip_quic_rx_ack", "ptls_hip_quic_rx_ack_timing")
STATUS = (("OK", 0), ("NO_CONN", 1), ("EMPTY", 2), ("STATE", 3))
PARAMS = ("d_spaces", "count", "space", "max_ranges", "ack_delay", "d_frames", "frames_len", "in_off", "pkt_base", "pkt_stride", "d_status",
          "d_frame_off", "d_frame_len", "d_reqs")


def _header():
    with open(os.path.join(ROOT, "include", "ptls_hip.h")) as f:
        return f.read()


def test_library_exports_the_ack_symbols():
    L = ptls_hip.lib()
    header = _header()
    for name in FUNCTIONS:
        assert hasattr(L, name), name
        assert name in ptls_hip.SIGNATURES, name
    decl = re.search(r"int ptls_hip_quic_rx_ack\(([^;]*)\);", header).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["rx", "params", "d_list", "n", "report", "stream"]
    res, args = ptls_hip.SIGNATURES["ptls_hip_quic_rx_ack"]
    assert res is ctypes.c_int and len(args) == 6 and args[3] is ctypes.c_size_t
    assert "void ptls_hip_quic_rx_ack_timing(float *ack_ms);" in header
    assert ptls_hip.SIGNATURES["ptls_hip_quic_rx_ack_timing"] == (None, [ctypes.POINTER(ctypes.c_float)])
    for name, value in STATUS:
        assert re.search(r"#define PTLS_HIP_QUIC_ACK_%s %du\b" % (name, value), header), name
        assert getattr(ptls_hip, "QUIC_ACK_" + name) == value
    assert re.search(r"#define PTLS_HIP_QUIC_ACK_MAX 81\b", header) and ptls_hip.QUIC_ACK_MAX == 81


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layouts_match_the_header(tmp_path):
    fields = {"ptls_hip_quic_rx_ack_t": PARAMS, "ptls_hip_quic_rx_ack_report_t": ("n_frames", "bytes")}
    body = "".join('    printf("%%zu%s\\n", sizeof(%s)%s);\n' % (" %zu" * len(fs), t, "".join(", offsetof(%s, %s)" % (t, f) for f in fs))
                   for t, fs in fields.items())
    body += '    printf("%s %%d\\n", %s, PTLS_HIP_QUIC_ACK_MAX);\n' % (" ".join(["%u"] * len(STATUS)),
                                                                     ", ".join("PTLS_HIP_QUIC_ACK_" + n for n, _ in STATUS))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptls_hip.h"\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    rows = [[int(x) for x in ln.split()] for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    P, T = ptls_hip.QuicRxAck, ptls_hip.QuicRxAckReport
    assert [f for f, _ in P._fields_] == list(PARAMS)
    assert rows[0] == [ctypes.sizeof(P)] + [getattr(P, f).offset for f in PARAMS] == [104, 0, 8, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96]
    assert rows[1] == [ctypes.sizeof(T), T.n_frames.offset, T.bytes.offset] == [16, 0, 8]
    assert rows[2] == [v for _, v in STATUS] + [81]


def test_refusals_without_a_device():
    L = ptls_hip.lib()
    fake = ctypes.create_string_buffer(256)  # an "engine": never dereferenced before the checks pass
    rx = L.ptls_hip_quic_rx_new(ctypes.addressof(fake), 0, 4)
    assert rx
    buf = 0x10000  # "device" addresses: never read by the host
    top = (1 << 64) - 1
    try:
        rep = ptls_hip.QuicRxAckReport(77, 77)
        base = dict(d_spaces=buf, count=8, space=2, max_ranges=31, ack_delay=0, d_frames=buf, frames_len=81 * 4, in_off=0, pkt_base=0,
                    pkt_stride=0, d_status=buf, d_frame_off=buf, d_frame_len=buf, d_reqs=buf)

        def ack(obj=rx, null_params=False, d_list=buf, n=4, report=rep, **kw):
            p = ptls_hip.QuicRxAck(*[dict(base, **kw)[f] for f in PARAMS])
            return L.ptls_hip_quic_rx_ack(obj, None if null_params else ctypes.addressof(p), d_list, n,
                                          ctypes.addressof(report) if report is not None else None, None)

        def refused(msg, **kw):
            assert ack(**kw) == ptls_hip.EINVAL, kw
            assert ptls_hip.last_error().startswith("quic_rx_ack: ") and msg in ptls_hip.last_error(), (kw, ptls_hip.last_error())
            assert (rep.n_frames, rep.bytes) == (77, 77)  # nothing written by a refused call

        for kw in (dict(obj=None), dict(null_params=True), dict(report=None)):
            refused("null receive object, parameters or report", **kw)
        for field in ("d_spaces", "d_status", "d_frame_off", "d_frame_len", "d_reqs"):
            refused("null state, status, frame-offset, frame-length or request array", **{field: None})
            refused("null state, status, frame-offset, frame-length or request array", n=0, **{field: None})
        refused("null list or frame buffer", d_list=None)
        refused("null list or frame buffer", d_frames=None)
        for count in (0, 1 << 32):
            refused("a connection count of %d is outside 1 .. 2^32 - 1" % count, count=count)
        refused("packet-number space 3 is above 2", space=3)
        refused("packet-number space 4294967295 is above 2", space=0xFFFFFFFF)
        refused("an ack_delay of 4611686018427387904 is not below 2^62", ack_delay=1 << 62)
        refused("an ack_delay of 18446744073709551615 is not below 2^62", ack_delay=top)
        most = 0xFFFFFFFF // 81
        refused("%d list entries: 81 bytes each do not fit the 32-bit scan levels" % (most + 1), n=most + 1, frames_len=top)
        refused("a frame buffer of %d bytes is below 81 for each of the %d list entries" % (81 * most - 1, most), n=most,
                frames_len=81 * most - 1)
        refused("a frame buffer of 323 bytes is below 81 for each of the 4 list entries", frames_len=323)
        refused("a frame buffer of 0 bytes", frames_len=0, n=1)
        refused("in_off plus 81 bytes for each of the 4 list entries wraps 2^64", in_off=top - 323)
        refused("pkt_base plus 4 packets of stride 4611686018427387904 wraps 2^64", pkt_stride=1 << 62)
        refused("pkt_base plus 4 packets of stride 1 wraps 2^64", pkt_base=top - 3, pkt_stride=1)
        # nothing listed: 0 with both sums 0, whatever the list and the frame buffer are
        assert ack(n=0, d_list=None, d_frames=None, frames_len=0, in_off=top, pkt_base=top, pkt_stride=top, max_ranges=0xFFFFFFFF,
                   ack_delay=(1 << 62) - 1) == 0
        assert (rep.n_frames, rep.bytes) == (0, 0)
        L.ptls_hip_quic_rx_ack_timing(None)  # no output asked for: a no-op
        t = ctypes.c_float(-1)
        L.ptls_hip_quic_rx_ack_timing(ctypes.byref(t))
        assert t.value == 0  # nothing was timed on this thread
    finally:
        L.ptls_hip_quic_rx_free(rx)
