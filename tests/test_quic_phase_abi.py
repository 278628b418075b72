"""CPU tests of the key-phase surface (include/ptls_hip.h 2j): the library exports the entry points and the binding declares
them, the two structs' layouts match the header, and every refusal that can be reached without a device fails with its
message and launches nothing: the engine pointer is never dereferenced and the "keysets" are never read before the checks in
front of them pass.  The refusal that needs a real keyset (three banks that do not fit it) lives in
tests/test_gpu_quic_keyphase.py."""
import ctypes
import os
import shutil
import subprocess

import pytest

import ptls_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("ptls_hip_quic_rx_open_keyphase", "ptls_hip_quic_rx_keyphase_commit", "ptls_hip_quic_rx_keyphase_timing")


def test_library_exports_the_keyphase_symbols():
    L = ptls_hip.lib()
    with open(os.path.join(ROOT, "include", "ptls_hip.h")) as f:
        header = f.read()
    for name in FUNCTIONS:
        assert hasattr(L, name), name
        assert name in ptls_hip.SIGNATURES, name
        assert name + "(" in header, name
    assert len(ptls_hip.SIGNATURES["ptls_hip_quic_rx_open_keyphase"][1]) == 14
    assert len(ptls_hip.SIGNATURES["ptls_hip_quic_rx_keyphase_commit"][1]) == 9
    assert "#define PTLS_HIP_QUIC_NO_GEN 0xffffffffu" in header and ptls_hip.QUIC_NO_GEN == 0xFFFFFFFF


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptls_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu\\n", sizeof(ptls_hip_quic_keyphase_t), offsetof(ptls_hip_quic_keyphase_t, first_pn),\n'
                   '           offsetof(ptls_hip_quic_keyphase_t, gen), offsetof(ptls_hip_quic_keyphase_t, reserved));\n'
                   '    printf("%zu %zu %zu %zu %zu\\n", sizeof(ptls_hip_quic_rx_keyphase_t), offsetof(ptls_hip_quic_rx_keyphase_t, d_phase),\n'
                   '           offsetof(ptls_hip_quic_rx_keyphase_t, count), offsetof(ptls_hip_quic_rx_keyphase_t, stride),\n'
                   '           offsetof(ptls_hip_quic_rx_keyphase_t, d_gen_out));\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = ptls_hip.QUIC_KEYPHASE_DTYPE
    assert out[:4] == [D.itemsize, D.fields["first_pn"][1], D.fields["gen"][1], D.fields["reserved"][1]] == [16, 0, 8, 12]
    K = ptls_hip.QuicRxKeyphase
    assert out[4:] == [ctypes.sizeof(K), K.d_phase.offset, K.count.offset, K.stride.offset, K.d_gen_out.offset] == [32, 0, 8, 16, 24]


def _fake():
    return ctypes.create_string_buffer(256)  # never dereferenced before the checks pass


def test_refusals_without_a_device():
    L = ptls_hip.lib()
    fake, ks, hp = _fake(), _fake(), _fake()
    rx = L.ptls_hip_quic_rx_new(ctypes.addressof(fake), 0, 4)
    assert rx
    buf = 0x1000  # a "device" address: never read by the host
    try:
        rep = ptls_hip.QuicRxReport(5, 5, 5)
        k, h, r = ctypes.addressof(ks), ctypes.addressof(hp), ctypes.addressof(rep)

        def open_kp(obj=rx, a=k, b=h, kp=(buf, 8, 8, buf), report=r):
            s = ptls_hip.QuicRxKeyphase(*kp) if kp is not None else None
            return L.ptls_hip_quic_rx_open_keyphase(obj, a, b, 0xFF, ctypes.addressof(s) if s is not None else None, buf, 16, buf + 64, 16,
                                                    buf, buf, buf, report, None)

        for kw, msg in ((dict(kp=None), "null key-phase parameters"), (dict(obj=None), "null receive object, keyset or report"),
                        (dict(a=None), "null receive object, keyset or report"), (dict(b=None), "null receive object, keyset or report"),
                        (dict(report=None), "null receive object, keyset or report"),
                        (dict(kp=(None, 8, 8, buf)), "null key-phase state or generation array"),
                        (dict(kp=(buf, 8, 8, None)), "null key-phase state or generation array"),
                        (dict(kp=(buf, 0, 8, buf)), "a bank stride or a state count of 0"),
                        (dict(kp=(buf, 8, 0, buf)), "a bank stride or a state count of 0")):
            assert open_kp(**kw) == ptls_hip.EINVAL, kw
            assert "quic_rx_open_keyphase:" in ptls_hip.last_error() and msg in ptls_hip.last_error(), (kw, ptls_hip.last_error())
        assert L.ptls_hip_quic_rx_set_plan(rx, ptls_hip.QUIC_RX_PLAN_HOST) == 0
        assert open_kp() == ptls_hip.EINVAL and "the host plan (rx_set_plan 2) fixes a chunk's key on the host" in ptls_hip.last_error()
        assert L.ptls_hip_quic_rx_set_plan(rx, ptls_hip.QUIC_RX_PLAN_AUTO) == 0
        assert (rep.n_selected, rep.planned_on_device, rep.lanes) == (5, 5, 5)  # nothing written by a refused call

        n_upd = ctypes.c_size_t(77)

        def commit(obj=rx, phase=buf, count=8, res=buf, pn=buf, gen=buf, upd=buf, n=n_upd):
            return L.ptls_hip_quic_rx_keyphase_commit(obj, phase, count, res, pn, gen, upd, ctypes.byref(n) if n is not None else None,
                                                      None)

        for kw in (dict(obj=None), dict(phase=None), dict(res=None), dict(pn=None), dict(gen=None), dict(upd=None), dict(n=None)):
            assert commit(**kw) == ptls_hip.EINVAL, kw
            assert "quic_rx_keyphase_commit: null receive object, state, array or n_updated" in ptls_hip.last_error()
        for count in (0, 1 << 32):
            assert commit(count=count) == ptls_hip.EINVAL and "is outside 1 .. 2^32 - 1" in ptls_hip.last_error()
        assert commit() == ptls_hip.EINVAL and "no rx_open_keyphase on the object" in ptls_hip.last_error()
        assert n_upd.value == 77
        L.ptls_hip_quic_rx_keyphase_timing(None, None)  # no output asked for: a no-op
        hm, cm = ctypes.c_float(-1), ctypes.c_float(-1)
        L.ptls_hip_quic_rx_keyphase_timing(ctypes.byref(hm), ctypes.byref(cm))
        assert hm.value == 0 and cm.value == 0  # nothing was timed on this thread
    finally:
        L.ptls_hip_quic_rx_free(rx)
