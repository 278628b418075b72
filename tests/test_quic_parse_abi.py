"""CPU tests of the datagram-parsing surface of libptls_hip.so (include/ptls_hip.h 2h): the library exports the entry points
and the binding declares them, the three struct layouts match the header (checked against a C compiler's offsetof), the
constants match, and every refusal that needs no device fails with its message, behind an engine pointer that is never
dereferenced before the checks pass (a connection-ID map allocates its device table with its first upload)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptls_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("ptls_hip_quic_cidmap_new", "ptls_hip_quic_cidmap_free", "ptls_hip_quic_cidmap_size", "ptls_hip_quic_cidmap_set",
             "ptls_hip_quic_cidmap_remove", "ptls_hip_quic_parse_datagrams", "ptls_hip_quic_parse_timing")
LAYOUTS = {
    "ptls_hip_quic_datagram_t": (16, (("off", 0), ("len", 8), ("reserved", 12))),
    "ptls_hip_quic_pktinfo_t": (32, (("dgram", 0), ("version", 4), ("conn", 8), ("token_len", 12), ("dcid_off", 16), ("scid_off", 18),
                                     ("token_off", 20), ("dcid_len", 22), ("scid_len", 23), ("type", 24), ("status", 25),
                                     ("flags", 26), ("pad", 27))),
    "ptls_hip_quic_parse_params_t": (32, (("short_cid_len", 0), ("max_per_dgram", 4), ("require_fixed_bit", 8), ("reserved", 12),
                                          ("d_expected_pn", 16), ("expected_count", 24))),
}
CONSTANTS = {"TYPE_INITIAL": 0, "TYPE_ZERO_RTT": 1, "TYPE_HANDSHAKE": 2, "TYPE_RETRY": 3, "TYPE_ONE_RTT": 4,
             "TYPE_VERSION_NEGOTIATION": 5, "TYPE_UNKNOWN_VERSION": 6, "TYPE_NONE": 7, "STATUS_OK": 0, "STATUS_TRUNCATED": 1,
             "STATUS_TOO_SHORT": 2, "STATUS_BAD_CID_LEN": 3, "STATUS_BAD_FIXED_BIT": 4, "INFO_MORE": 1, "NO_CONN": 0xFFFFFFFF}


def test_library_exports_the_parse_symbols():
    L = ptls_hip.lib()
    with open(os.path.join(ROOT, "include", "ptls_hip.h")) as f:
        header = f.read()
    for name in FUNCTIONS:
        assert hasattr(L, name), name
        assert name in ptls_hip.SIGNATURES, name
        assert name + "(" in header, name
    assert len(ptls_hip.SIGNATURES["ptls_hip_quic_parse_datagrams"][1]) == 12
    for name, value in CONSTANTS.items():
        assert getattr(ptls_hip, "QUIC_" + name) == value, name
        text = "0x%xu" % value if value > 255 else "%du" % value
        assert "#define PTLS_HIP_QUIC_%s %s" % (name, text) in header, name


def test_dtype_layouts():
    for dt, name in ((ptls_hip.QUIC_DATAGRAM_DTYPE, "ptls_hip_quic_datagram_t"), (ptls_hip.QUIC_PKTINFO_DTYPE, "ptls_hip_quic_pktinfo_t")):
        size, fields = LAYOUTS[name]
        assert dt.itemsize == size and dt.names == tuple(n for n, _ in fields)
        assert tuple(dt.fields[n][1] for n, _ in fields) == tuple(o for _, o in fields)
    P = ptls_hip.QuicParseParams
    size, fields = LAYOUTS["ptls_hip_quic_parse_params_t"]
    assert ctypes.sizeof(P) == size and [(n, getattr(P, n).offset) for n, _ in P._fields_] == list(fields)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_layouts_match_the_header(tmp_path):
    lines = []
    for name, (_, fields) in LAYOUTS.items():
        lines.append('    printf("%%zu", sizeof(%s));\n' % name)
        lines += ['    printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f, _ in fields]
        lines.append('    printf("\\n");\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptls_hip.h"\nint main(void) {\n' + "".join(lines) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    want = [[size] + [o for _, o in fields] for size, fields in LAYOUTS.values()]
    assert [[int(x) for x in ln.split()] for ln in out] == want


def _fake_engine():
    return ctypes.create_string_buffer(256)  # never dereferenced before the checks pass


def _cids(*cids):
    return b"".join(c[:20].ljust(20, b"\0") for c in cids), bytes(len(c) for c in cids)


def test_cidmap_refusals_without_a_device():
    L = ptls_hip.lib()
    fake = _fake_engine()
    eng = ctypes.addressof(fake)
    assert L.ptls_hip_quic_cidmap_new(None, 8) is None and "quic_cidmap_new" in ptls_hip.last_error()
    assert L.ptls_hip_quic_cidmap_new(eng, 0) is None and "capacity 0" in ptls_hip.last_error()
    assert L.ptls_hip_quic_cidmap_new(eng, (1 << 30) + 1) is None and "outside 1 .. 2^30" in ptls_hip.last_error()
    L.ptls_hip_quic_cidmap_free(None)  # a no-op
    assert L.ptls_hip_quic_cidmap_size(None) == 0
    m = L.ptls_hip_quic_cidmap_new(eng, 2)
    assert m
    try:
        packed, lens = _cids(b"abc", b"12345678")
        conns = np.array([1, 2], dtype=np.uint32)
        assert L.ptls_hip_quic_cidmap_set(None, 2, packed, lens, conns.ctypes.data, None) == ptls_hip.EINVAL
        assert "quic_cidmap_set: null map" in ptls_hip.last_error()
        assert L.ptls_hip_quic_cidmap_remove(None, 2, packed, lens, None) == ptls_hip.EINVAL
        assert "quic_cidmap_remove: null map" in ptls_hip.last_error()
        for args in ((None, lens, conns.ctypes.data), (packed, None, conns.ctypes.data), (packed, lens, None)):
            assert L.ptls_hip_quic_cidmap_set(m, 2, *args, None) == ptls_hip.EINVAL
            assert "quic_cidmap_set: null" in ptls_hip.last_error()
        assert L.ptls_hip_quic_cidmap_remove(m, 2, None, lens, None) == ptls_hip.EINVAL
        assert L.ptls_hip_quic_cidmap_remove(m, 2, packed, None, None) == ptls_hip.EINVAL
        # a length above 20, in either call; the message names the index
        assert L.ptls_hip_quic_cidmap_set(m, 2, packed, bytes([3, 21]), conns.ctypes.data, None) == ptls_hip.EINVAL
        assert "cid_lens[1] is 21" in ptls_hip.last_error()
        assert L.ptls_hip_quic_cidmap_remove(m, 2, packed, bytes([255, 8]), None) == ptls_hip.EINVAL
        assert "cid_lens[0] is 255" in ptls_hip.last_error()
        # the value that means no connection
        bad = np.array([1, 0xFFFFFFFF], dtype=np.uint32)
        assert L.ptls_hip_quic_cidmap_set(m, 2, packed, lens, bad.ctypes.data, None) == ptls_hip.EINVAL
        assert "conns[1] is 0xffffffff" in ptls_hip.last_error()
        # more new CIDs than the capacity (the same CID twice counts once: that call would get as far as the device)
        packed3, lens3 = _cids(b"abc", b"12345678", b"")
        three = np.array([1, 2, 3], dtype=np.uint32)
        assert L.ptls_hip_quic_cidmap_set(m, 3, packed3, lens3, three.ctypes.data, None) == ptls_hip.EINVAL
        assert "exceed the capacity of 2" in ptls_hip.last_error()
        assert L.ptls_hip_quic_cidmap_size(m) == 0  # nothing changed in any of them
        assert L.ptls_hip_quic_cidmap_set(m, 0, None, None, None, None) == 0
        assert L.ptls_hip_quic_cidmap_remove(m, 0, None, None, None) == 0
        assert L.ptls_hip_quic_cidmap_remove(m, 2, packed, lens, None) == 0  # absent CIDs: nothing to upload
    finally:
        L.ptls_hip_quic_cidmap_free(m)  # no device table was ever allocated


def _params(**kw):
    p = ptls_hip.QuicParseParams(8, 16, 1, 0, None, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_parse_refusals_without_a_device():
    L = ptls_hip.lib()
    fake, other = _fake_engine(), _fake_engine()
    eng = ctypes.addressof(fake)
    dg = np.zeros(3, dtype=ptls_hip.QUIC_DATAGRAM_DTYPE)
    dg["off"], dg["len"] = (0, 100, 200), (100, 100, 56)
    sentinel = 0xA5
    pkts = np.full(4, sentinel, dtype=np.uint8).repeat(40).view(ptls_hip.QUIC_PACKET_DTYPE)
    info = np.full(4, sentinel, dtype=np.uint8).repeat(32).view(ptls_hip.QUIC_PKTINFO_DTYPE)
    n_pkts = ctypes.c_size_t(77)
    buf = 0x1000  # a "device" address: never read by the host

    def call(engine=eng, params=None, cmap=None, dgrams=dg, n=3, d_buf=buf, buf_len=256, h_pkts=pkts, h_info=info, cap=4, out=n_pkts):
        p = params if params is not None else _params()
        return L.ptls_hip_quic_parse_datagrams(engine, ctypes.addressof(p) if p is not False else None, cmap,
                                               dgrams.ctypes.data if dgrams is not None else None, n, d_buf, buf_len,
                                               h_pkts.ctypes.data if h_pkts is not None else None,
                                               h_info.ctypes.data if h_info is not None else None, cap,
                                               ctypes.byref(out) if out is not None else None, None)

    for kw, msg in ((dict(engine=None), "null engine"), (dict(params=False), "null engine, parameters"), (dict(out=None), "n_pkts"),
                    (dict(dgrams=None), "null datagram array or buffer"), (dict(d_buf=None), "null datagram array or buffer"),
                    (dict(h_pkts=None), "null output array"), (dict(h_info=None), "null output array"),
                    (dict(params=_params(short_cid_len=21)), "short_cid_len 21 is above 20"),
                    (dict(params=_params(max_per_dgram=0)), "max_per_dgram 0 is outside 1..16"),
                    (dict(params=_params(max_per_dgram=17)), "max_per_dgram 17 is outside 1..16"),
                    (dict(params=_params(reserved=1)), "reserved must be 0"),
                    (dict(n=1 << 32), "above 2^32 - 1"), (dict(n=1 << 28), "above 2^32 - 1"),
                    (dict(buf_len=255), "datagram 2: off 200 + len 56 is past the buffer of 255 bytes")):
        assert call(**kw) == ptls_hip.EINVAL, kw
        assert "quic_parse_datagrams:" in ptls_hip.last_error() and msg in ptls_hip.last_error(), (kw, ptls_hip.last_error())
    big = dg.copy()
    big["len"][1] = 65536
    assert call(dgrams=big, buf_len=1 << 20) == ptls_hip.EINVAL
    assert "datagram 1: len 65536 is above 65535" in ptls_hip.last_error()
    far = dg.copy()
    far["off"][0] = (1 << 64) - 50  # off + len wraps
    assert call(dgrams=far) == ptls_hip.EINVAL and "datagram 0:" in ptls_hip.last_error()
    m = L.ptls_hip_quic_cidmap_new(ctypes.addressof(other), 4)
    try:
        assert call(cmap=m) == ptls_hip.EINVAL
        assert "belongs to another engine" in ptls_hip.last_error()
    finally:
        L.ptls_hip_quic_cidmap_free(m)
    # nothing was written by any of them
    assert n_pkts.value == 77
    assert (pkts.view(np.uint8) == sentinel).all() and (info.view(np.uint8) == sentinel).all()
    # n == 0: fine without a device, whatever the other pointers are
    assert call(n=0, dgrams=None, d_buf=None, h_pkts=None, h_info=None, cap=0) == 0 and n_pkts.value == 0
