"""Builds tests/device_harness.hip (the product's device code behind small test kernels) for gfx950 into
tests/_build/libcvdev.so with the product's own compiler flags (corda_amd/build.py).  Cross-compiles without a GPU.
The file is compiled as five translation units side by side (-DCVD_PART=1..5: see the source), rebuilt when
the source, this file or any corda_amd/csrc header is newer than the library."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from corda_amd import build as product  # noqa: E402

SRC = os.path.join(REPO, "tests", "device_harness.hip")
OUT = os.path.join(REPO, "tests", "_build")
LIB = os.path.join(OUT, "libcvdev.so")
PARTS = (1, 2, 3, 4, 5)


def build() -> str:
    csrc = product.CSRC
    deps = [SRC, os.path.abspath(__file__), os.path.abspath(product.__file__)]
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    os.makedirs(OUT, exist_ok=True)
    objs = [os.path.join(OUT, f"cvdev_{p}.o") for p in PARTS]
    cmds = [[product.HIPCC] + product.CFLAGS + product.KERNEL_FLAGS + [f"-DCVD_PART={p}", "-c", SRC, "-o", o]
            for p, o in zip(PARTS, objs)]
    with ThreadPoolExecutor(len(cmds)) as pool:
        for r in pool.map(lambda c: subprocess.run(c, capture_output=True, text=True), cmds):
            if r.returncode:
                sys.stderr.write(r.stderr)
                raise subprocess.CalledProcessError(r.returncode, r.args)
    subprocess.run([product.HIPCC, f"--offload-arch={product.ARCH}", "-shared", "-fPIC", "-o", LIB] + objs, check=True)
    return LIB


if __name__ == "__main__":
    print(build())
