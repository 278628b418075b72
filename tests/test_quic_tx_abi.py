"""CPU tests of the send object's surface (include/ptls_hip.h 2l): the library exports the entry points and the binding
declares them with the header's signatures, the structs' layouts and the status constants match the header, and every refusal
fails with its message, launches nothing and writes nothing: none of them needs a device."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import ptls_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("ptls_hip_quic_tx_new", "ptls_hip_quic_tx_free", "ptls_hip_quic_tx_seal", "ptls_hip_quic_tx_packets",
             "ptls_hip_quic_tx_count", "ptls_hip_quic_tx_timing")
STATUS = (("SENT", 0), ("NO_CONN", 1), ("SPLIT", 2), ("PN", 3), ("RANGE", 4))


def _header():
    with open(os.path.join(ROOT, "include", "ptls_hip.h")) as f:
        return f.read()


def test_library_exports_the_send_symbols():
    L = ptls_hip.lib()
    header = _header()
    for name in FUNCTIONS:
        assert hasattr(L, name), name
        assert name in ptls_hip.SIGNATURES, name
    decl = re.search(r"int ptls_hip_quic_tx_seal\(([^;]*)\);", header).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["tx", "ks", "hp_ks", "params", "d_reqs", "n", "d_in", "in_len", "d_pkt",
                                                                  "buf_len", "report", "stream"]
    res, args = ptls_hip.SIGNATURES["ptls_hip_quic_tx_seal"]
    assert res is ctypes.c_int and len(args) == 12 and [args[k] for k in (5, 7, 9)] == [ctypes.c_size_t] * 3
    assert "ptls_hip_quic_tx_t *ptls_hip_quic_tx_new(ptls_hip_engine_t *engine, size_t cap);" in header
    assert ptls_hip.SIGNATURES["ptls_hip_quic_tx_new"] == (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_size_t])
    assert "void ptls_hip_quic_tx_timing(int enable, float *front_ms, float *sort_ms);" in header
    assert ptls_hip.SIGNATURES["ptls_hip_quic_tx_timing"] == (None, [ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                                                     ctypes.POINTER(ctypes.c_float)])
    for name, value in STATUS:
        assert re.search(r"#define PTLS_HIP_QUIC_TX_%s %du\b" % (name, value), header), name
        assert getattr(ptls_hip, "QUIC_TX_" + name) == value


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layouts_match_the_header(tmp_path):
    fields = {"ptls_hip_quic_txconn_t": ("next_pn", "largest_acked", "gen", "dcid_len", "flags", "reserved", "dcid", "reserved2"),
              "ptls_hip_quic_txreq_t": ("data_off", "pkt_off", "conn", "len"),
              "ptls_hip_quic_tx_params_t": ("d_conns", "count", "stride", "d_rx_phase", "pn_len", "reserved", "d_status", "d_pn_out",
                                            "d_pkt_len"),
              "ptls_hip_quic_tx_report_t": ("n_sent", "bytes", "lanes", "reserved")}
    body = "".join('    printf("%%zu%s\\n", sizeof(%s)%s);\n' % (" %zu" * len(fs), t, "".join(", offsetof(%s, %s)" % (t, f) for f in fs))
                   for t, fs in fields.items())
    body += '    printf("%s\\n", %s);\n' % (" ".join(["%u"] * len(STATUS)), ", ".join("PTLS_HIP_QUIC_TX_" + n for n, _ in STATUS))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptls_hip.h"\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    rows = [[int(x) for x in ln.split()] for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    C, R = ptls_hip.QUIC_TXCONN_DTYPE, ptls_hip.QUIC_TXREQ_DTYPE
    assert rows[0] == [C.itemsize] + [C.fields[f][1] for f in fields["ptls_hip_quic_txconn_t"]] == [48, 0, 8, 16, 20, 21, 22, 24, 44]
    assert rows[1] == [R.itemsize] + [R.fields[f][1] for f in fields["ptls_hip_quic_txreq_t"]] == [24, 0, 8, 16, 20]
    P, T = ptls_hip.QuicTxParams, ptls_hip.QuicTxReport
    assert rows[2] == [ctypes.sizeof(P)] + [getattr(P, f).offset for f in fields["ptls_hip_quic_tx_params_t"]] == \
        [64, 0, 8, 16, 24, 32, 36, 40, 48, 56]
    assert rows[3] == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields["ptls_hip_quic_tx_report_t"]] == [24, 0, 8, 16, 20]
    assert rows[4] == [v for _, v in STATUS]


class FakeKeyset(ctypes.Structure):
    """the head of st_ptls_hip_keyset_t (csrc/host.h) as the refusals read it: engine, key size, slots, algorithm"""
    _fields_ = [("eng", ctypes.c_void_p), ("key_size", ctypes.c_size_t), ("nslots", ctypes.c_size_t), ("algo", ctypes.c_int)]


def test_refusals_without_a_device():
    L = ptls_hip.lib()
    fake = ctypes.create_string_buffer(256)  # an "engine": never dereferenced before the checks pass
    other = ctypes.create_string_buffer(256)
    eng = ctypes.addressof(fake)
    assert not L.ptls_hip_quic_tx_new(None, 4) and "quic_tx_new: null engine, or cap 4 outside" in ptls_hip.last_error()
    for cap in (0, 1 << 32):
        assert not L.ptls_hip_quic_tx_new(eng, cap) and "cap %d outside 1 .. 2^32 - 1" % cap in ptls_hip.last_error()
    tx = L.ptls_hip_quic_tx_new(eng, 4)
    assert tx
    buf = 0x10000  # "device" addresses: never read by the host
    ks = FakeKeyset(eng, 16, 30, ptls_hip.ALGO_AESGCM)
    hp = FakeKeyset(eng, 16, 10, ptls_hip.ALGO_AESGCM)
    try:
        rep = ptls_hip.QuicTxReport(77, 77, 77, 77)

        def seal(obj=tx, keys=ks, hps=hp, pr=(buf, 8, 10, None, 0, 0, buf, buf, buf), reqs=buf, n=4, d_in=buf, in_len=256,
                 d_pkt=buf + 4096, buf_len=256, report=rep):
            p = ptls_hip.QuicTxParams(*pr) if pr is not None else None
            return L.ptls_hip_quic_tx_seal(obj, ctypes.addressof(keys) if keys is not None else None,
                                           ctypes.addressof(hps) if hps is not None else None, ctypes.addressof(p) if p is not None else None,
                                           reqs, n, d_in, in_len, d_pkt, buf_len, ctypes.addressof(report) if report is not None else None,
                                           None)

        def refused(msg, **kw):
            assert seal(**kw) == ptls_hip.EINVAL, kw
            assert ptls_hip.last_error().startswith("quic_tx_seal: ") and msg in ptls_hip.last_error(), (kw, ptls_hip.last_error())
            assert (rep.n_sent, rep.bytes, rep.lanes, rep.reserved) == (77, 77, 77, 77)  # nothing written by a refused call

        for kw in (dict(obj=None), dict(keys=None), dict(hps=None), dict(pr=None), dict(report=None)):
            refused("null send object, keyset, parameters or report", **kw)
        for k in (0, 6, 7, 8):
            pr = [buf, 8, 10, None, 0, 0, buf, buf, buf]
            pr[k] = None
            refused("null state, status, packet-number or packet-length array", pr=tuple(pr))
        refused("5 requests, the send object was made for 4", n=5)
        for count in (0, 1 << 32):
            refused("a state count of %d is outside 1 .. 2^32 - 1" % count, pr=(buf, count, 10, None, 0, 0, buf, buf, buf))
        refused("a bank stride of 0", pr=(buf, 8, 0, None, 0, 0, buf, buf, buf))
        refused("pn_len 5 is above 4", pr=(buf, 8, 10, None, 5, 0, buf, buf, buf))
        refused("params.reserved is not 0", pr=(buf, 8, 10, None, 0, 1, buf, buf, buf))
        refused("must belong to the same engine", keys=FakeKeyset(ctypes.addressof(other), 16, 30, ptls_hip.ALGO_AESGCM))
        refused("must belong to the same engine", hps=FakeKeyset(ctypes.addressof(other), 16, 10, ptls_hip.ALGO_AESGCM))
        refused("algorithm and key size", hps=FakeKeyset(eng, 32, 10, ptls_hip.ALGO_AESGCM))
        refused("algorithm and key size", hps=FakeKeyset(eng, 16, 10, ptls_hip.ALGO_CHACHA20POLY1305))
        refused("three banks of stride 11 do not fit the keyset's 30 slots", pr=(buf, 8, 11, None, 0, 0, buf, buf, buf))
        for kw in (dict(reqs=None), dict(d_in=None), dict(d_pkt=None)):
            refused("null request array or buffer", **kw)
        for d_pkt, buf_len in ((buf, 256), (buf + 255, 16), (buf - 15, 16), (buf - 100, 1000)):
            refused("the packet buffer overlaps the payload buffer", d_pkt=d_pkt, buf_len=buf_len)
        # nothing to send: 0 with a zeroed report, whatever the request array and the buffers are
        assert seal(n=0, reqs=None, d_in=None, d_pkt=None) == 0
        assert (rep.n_sent, rep.bytes, rep.lanes, rep.reserved) == (0, 0, 0, 0)
        assert L.ptls_hip_quic_tx_count(tx) == 0 and not L.ptls_hip_quic_tx_packets(tx)
        assert L.ptls_hip_quic_tx_count(None) == 0 and not L.ptls_hip_quic_tx_packets(None)
        L.ptls_hip_quic_tx_timing(0, None, None)  # no output asked for: a no-op
        a, b = ctypes.c_float(-1), ctypes.c_float(-1)
        L.ptls_hip_quic_tx_timing(0, ctypes.byref(a), ctypes.byref(b))
        assert (a.value, b.value) == (0, 0)  # nothing was timed on this thread
    finally:
        L.ptls_hip_quic_tx_free(tx)
    L.ptls_hip_quic_tx_free(None)
