"""csrc/ctr_window.h (the batch kernel's counter-mode window constants) on the CPU, against plain FIPS-197 rounds.

The header compiles without HIP; tests/host_check/ctr_window_check.cpp includes it and the oracle's AES
(oracle/aesgcm_oracle.c) and checks, for 32 random (key, nonce) pairs of each key size and every block counter
2 .. 65535, that the state after round 2 from the window form equals two plain rounds, with the constants refreshed
exactly where the kernel refreshes them (every step KP * G and starting phase), for windows visited out of order, and that
a stale window is seen.  Built with AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program, nothing is loaded
into Python and no GPU is used."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_check", "ctr_window_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("gcc") is None, reason="g++ / gcc missing")
def test_window_form_equals_plain_rounds(tmp_path):
    obj, exe = str(tmp_path / "aesgcm_oracle.o"), str(tmp_path / "ctr_window_check")
    inc = ["-I" + os.path.join(ROOT, "hsig-picotls_amd", "csrc"), "-I" + os.path.join(ROOT, "oracle")]
    r = subprocess.run(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", *SAN, "-c",
                        os.path.join(ROOT, "oracle", "aesgcm_oracle.c"), "-o", obj], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-DGF128_FN=inline", *SAN, *inc, SRC, obj, "-o", exe, "-pthread"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, "32"], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "ctr_window_check: ok (0 failed of" in out and "32 pairs per key size" in out, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
