"""CPU tests of the QUIC packet-protection surface of libptls_hip.so (include/ptls_hip.h 2e): the library exports the entry
points and the binding declares them, QUIC_PACKET_DTYPE has the header's 40-byte layout (checked against a C compiler's
offsetof), and every refusal that needs no device fails with its message: a NULL engine or batch, and the host-checked
packet fields behind an engine pointer that is never dereferenced before they pass."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptls_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("ptls_hip_quic_batch_new", "ptls_hip_quic_batch_free", "ptls_hip_quic_batch_records", "ptls_hip_quic_seal_batch",
             "ptls_hip_quic_open_batch")
FIELDS = ("pkt_off", "data_off", "pn", "pkt_len", "key", "hp_key", "pn_offset", "pn_len", "flags")
OFFSETS = (0, 8, 16, 24, 28, 32, 36, 38, 39)


def test_library_exports_the_quic_symbols():
    L = ptls_hip.lib()
    for name in FUNCTIONS:
        assert hasattr(L, name), name
        assert name in ptls_hip.SIGNATURES, name
    assert ptls_hip.QUIC_UNPROTECTED == 1
    with open(os.path.join(ROOT, "include", "ptls_hip.h")) as f:
        header = f.read()
    assert "#define PTLS_HIP_QUIC_UNPROTECTED 1u" in header
    for name in FUNCTIONS:
        assert name + "(" in header, name


def test_packet_dtype_layout():
    dt = ptls_hip.QUIC_PACKET_DTYPE
    assert dt.itemsize == 40 and dt.names == FIELDS
    assert tuple(dt.fields[n][1] for n in FIELDS) == OFFSETS
    assert [dt.fields[n][0].itemsize for n in FIELDS] == [8, 8, 8, 4, 4, 4, 2, 1, 1]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_packet_dtype_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptls_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(ptls_hip_quic_packet_t));\n' +
                   "".join('    printf(" %%zu", offsetof(ptls_hip_quic_packet_t, %s));\n' % n for n in FIELDS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [40] + list(OFFSETS)


def _pkt(**kw):
    p = np.zeros(1, dtype=ptls_hip.QUIC_PACKET_DTYPE)
    p["pkt_len"], p["pn_offset"], p["pn_len"] = 1 + 4 + 16, 1, 1
    for k, v in kw.items():
        p[k] = v
    return p


def test_refusals_without_a_device():
    L = ptls_hip.lib()
    good = _pkt()
    # a NULL engine, a NULL descriptor array with n != 0, too many packets
    assert L.ptls_hip_quic_batch_new(None, good.ctypes.data, 1, 0, None) is None
    assert "quic_batch_new: bad arguments" in ptls_hip.last_error()
    fake = ctypes.create_string_buffer(256)  # never dereferenced before the packet checks pass
    eng = ctypes.addressof(fake)
    assert L.ptls_hip_quic_batch_new(eng, None, 1, 0, None) is None
    assert "quic_batch_new: bad arguments" in ptls_hip.last_error()
    assert L.ptls_hip_quic_batch_new(eng, good.ctypes.data, 1 << 32, 1, None) is None
    assert "quic_batch_new: bad arguments" in ptls_hip.last_error()
    # the host-checked packet fields, the offending packet at index 2 of 3: (fields, open, message)
    cases = [
        (dict(pn_offset=0, pkt_len=40), 0, "pn_offset is 0"),
        (dict(pn_offset=0, pkt_len=40), 1, "pn_offset is 0"),
        (dict(pn_len=0), 0, "pn_len must be 1..4"),
        (dict(pn_len=5, pkt_len=64), 0, "pn_len must be 1..4"),
        (dict(pn=1 << 62), 0, "below 2^62"),
        (dict(pn=(1 << 64) - 1), 0, "below 2^62"),
        (dict(pkt_len=20), 0, "pkt_len < pn_offset + 20"),
        (dict(pkt_len=20), 1, "pkt_len < pn_offset + 20"),
        (dict(pn_offset=47, pkt_len=66), 0, "pkt_len < pn_offset + 20"),
        (dict(pn_offset=47, pkt_len=66), 1, "pkt_len < pn_offset + 20"),
        (dict(pn_offset=65535, pkt_len=65554), 1, "pkt_len < pn_offset + 20"),
        (dict(pkt_len=0), 1, "pkt_len < pn_offset + 20"),
    ]
    for fields, is_open, msg in cases:
        pk = np.concatenate([good, good, _pkt(**fields)])
        assert L.ptls_hip_quic_batch_new(eng, pk.ctypes.data, 3, is_open, None) is None, fields
        err = ptls_hip.last_error()
        assert "quic_batch_new: packet 2:" in err and msg in err, (fields, err)
    # the calls on a NULL batch or NULL keysets
    assert L.ptls_hip_quic_batch_records(None) is None
    assert "null batch" in ptls_hip.last_error()
    assert L.ptls_hip_quic_seal_batch(None, eng, eng, eng, eng, None) == ptls_hip.EINVAL
    assert "quic_seal_batch: null batch or keyset" in ptls_hip.last_error()
    assert L.ptls_hip_quic_open_batch(None, eng, eng, eng, eng, eng, eng, None) == ptls_hip.EINVAL
    assert "quic_open_batch: null batch or keyset" in ptls_hip.last_error()
    L.ptls_hip_quic_batch_free(None)  # a no-op


def test_open_ignores_pn_len_and_pn_range():
    """open: pn_len is read from the packet and pn is the caller's expectation, so neither is a reason to refuse; the call
    gets as far as the engine (a NULL one here: the packet checks come after the argument check, so probe them one at a time
    through the message of a packet that is bad for another reason)"""
    L = ptls_hip.lib()
    fake = ctypes.create_string_buffer(256)
    pk = np.concatenate([_pkt(pn_len=0, pn=(1 << 64) - 1), _pkt(pn_len=9), _pkt(pkt_len=3)])
    assert L.ptls_hip_quic_batch_new(ctypes.addressof(fake), pk.ctypes.data, 3, 1, None) is None
    assert "quic_batch_new: packet 2:" in ptls_hip.last_error()  # not packet 0 or 1
