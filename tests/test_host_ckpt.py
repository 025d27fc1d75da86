"""The background checkpoint writer under the host sanitizers (CPU; no GPU, no HIP).

csrc/ckpt.cpp is the library's one piece of multi-threaded code and includes nothing of HIP,
so it is built here with plain clang++ together with the stand-alone driver
tests/host/ckpt_threads.cpp -- once with `-fsanitize=thread`, once with
`-fsanitize=address,undefined` -- and run as an ordinary executable.  Any sanitizer report
or failed check fails the test.  Skipped when clang++ is absent.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANGXX), reason="ROCm's clang++ absent")
@pytest.mark.parametrize("san", ["thread", "address,undefined"])
def test_ckpt_writer_sanitized(tmp_path, san):
    exe = tmp_path / "ckpt_threads"
    # no HIP include path: ckpt.cpp must build from the public header and err.h alone
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=" + san, "-pthread", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "hd-gnn_amd", "csrc"),
                    os.path.join(ROOT, "hd-gnn_amd", "csrc", "ckpt.cpp"),
                    os.path.join(ROOT, "tests", "host", "ckpt_threads.cpp"), "-o", str(exe)],
                   check=True, timeout=300)
    out = tmp_path / "out"
    out.mkdir()
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1",
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(out)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    for mark in ("WARNING: ThreadSanitizer", "ERROR: AddressSanitizer", "runtime error"):
        assert mark not in r.stderr, r.stderr[-4000:]
