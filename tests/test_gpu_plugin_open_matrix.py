"""The open-side authentication matrix through the plugin's single-record path (sparse_record one wave, mw_record two
waves, two pairs of waves at stride 128, the 16 KiB record; the ChaCha object), in its own process, with the resident
worker (default) and with one launch per call (PTLS_HIP_PLUGIN_WORKER=0): tests/plugin_open_matrix_case.py alternates the
valid record with requests that differ from it in one tag, ciphertext, AAD or sequence-number bit, in a length field or in
one static-IV bit, and compares every verdict with lib/fusion.c (oracle/_ref) or tests/chacha_ref.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("worker", ["1", "0"])
def test_plugin_open_matrix(worker):
    from oracle_lib import Ref
    if not Ref.available:
        pytest.skip("oracle/_ref not built")
    env = dict(os.environ, PTLS_HIP_PLUGIN_WORKER=worker)
    r = subprocess.run([sys.executable, os.path.join(HERE, "plugin_open_matrix_case.py")], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    # two calls per case (valid, then the case), 24 around the IV bits and a final one, per context and size
    import open_matrix as om
    import plugin_open_matrix_case as case
    n = 0
    for key_len in (16, 32):
        for N in case.AES_N:
            d = len(om.damages(om.aes_len_of_elements(N), om.AAD_LEN, key_len, "TCASL", c_every=16 if N > 1000 else 1))
            n += 2 * (d + (d + 2) // 3) + 25
    d = len(om.damages(case.CHACHA_LEN, om.AAD_LEN, 32, "TCASL", chacha=True))
    n += 2 * (d + (d + 2) // 3) + 25
    assert int(r.stdout.split()[1]) == n > 7000
