"""The one probe walk and the one size function of the device hash tables (corda_amd/csrc/cv_table.h) alone, on the
CPU, under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program (tests/table_san.cpp).  No GPU.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_sanitizers_standalone_program():
    """tests/table_san.cpp (its own main: the walk's order, bound, stop, wrap count and null counter over an exactly
    sized table, the size function against a restatement) under ASan + UBSan, run as a subprocess: nothing is loaded
    into this process under a sanitizer."""
    exe = os.path.join(REPO, "tests", "_build", "table_san")
    src = os.path.join(REPO, "tests", "table_san.cpp")
    deps = [src, os.path.join(REPO, "corda_amd", "csrc", "cv_table.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-O1", "-g", "-std=c++17",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                        "-Xarch_host", "-fno-omit-frame-pointer", src, "-o", exe, "-fsanitize=address,undefined"],
                       check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    for bad in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"):
        assert bad not in out, out[-4000:]
    assert r.stdout.split()[0] == "ok"
