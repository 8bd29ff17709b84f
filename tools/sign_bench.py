#!/usr/bin/env python3
"""Fixed-key signing against the per-message-key signer, same process, same inputs.

Device-resident 32-byte messages (tx ids) at n = 4,096 and 65,536:
  old    cv_ed25519_sign_device with the seed repeated n times (what BatchingNotary._sign used to call)
  keyed  cv_ed25519_sign_keyed_device with a cv_signer opened on that seed
timed with HIP events around a window of 2^21 signatures' worth of back-to-back calls on one stream, the two
paths alternating, `reps` repetitions each after a warm-up of both; median and spread (min, max, interquartile
range) per call.  The two paths' signatures are compared byte for byte at each size before anything is timed.
The host-buffer forms (Engine.sign_batch, Signer.sign: copies in, kernel, copy out, synchronous) are timed with
the host clock at the same sizes.  One more device-resident size, 2^20, fills the chip for several rounds of
waves: its rate is the throughput figure (the two sizes above fit one round, so theirs are a lane's latency).
Writes one JSON record (default profiles/sign_keyed.json).  Needs a GPU: no fallback.

    python tools/sign_bench.py [--reps 20] [--out profiles/sign_keyed.json]
    python tools/sign_bench.py --compiler-remarks     # adds the kernel's VGPRs / scratch / occupancy to the record
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from corda_amd import native  # noqa: E402

SIZES = (4096, 65536)
# both fit one round of the chip's resident waves (a call's time is one lane's chain); this one does not, so its
# signatures per second are a throughput figure (device-resident form only)
THROUGHPUT_SIZE = 1 << 20
MSG_LEN = 32


def spread(xs):
    xs = sorted(xs)
    q = statistics.quantiles(xs, n=4)
    return {"median_ms": statistics.median(xs), "min_ms": xs[0], "max_ms": xs[-1], "iqr_ms": q[2] - q[0],
            "reps": len(xs)}


def device_pair(engine, signer, seed, n, reps, warmup, stream):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(8032 + n)
    arena = torch.randint(0, 256, (n * MSG_LEN + 16,), dtype=torch.uint8, device=dev, generator=g)
    off = torch.arange(n, dtype=torch.int64, device=dev) * MSG_LEN
    ln = torch.full((n,), MSG_LEN, dtype=torch.int32, device=dev)
    seeds = torch.from_numpy(np.tile(np.frombuffer(seed, np.uint8), (n, 1))).to(dev)
    pk = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    sig_old = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    sig_new = torch.ones((n, 64), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    s = stream.cuda_stream

    def old():
        engine.sign_device(0, n, seeds.data_ptr(), arena.data_ptr(), off.data_ptr(), ln.data_ptr(), pk.data_ptr(),
                           sig_old.data_ptr(), s)

    def keyed():
        signer.sign_device(0, n, arena.data_ptr(), off.data_ptr(), ln.data_ptr(), sig_new.data_ptr(), s)

    old()
    keyed()
    stream.synchronize()
    if not torch.equal(sig_old, sig_new):
        raise SystemExit(f"n={n}: the keyed signatures differ from cv_ed25519_sign_device's")
    inner = max(1, (1 << 21) // n)                   # a timed window of 2^21 signatures: 7 ms to 0.6 s per window

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(inner):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / inner

    for _ in range(warmup):
        timed(old)
        timed(keyed)
    t_old, t_new = [], []
    for _ in range(reps):                            # interleaved: drift hits both alike
        t_old.append(timed(old))
        t_new.append(timed(keyed))
    so, sn = spread(t_old), spread(t_new)
    return {"n": n, "msg_len": MSG_LEN, "calls_per_window": inner, "old": so, "keyed": sn,
            "ratio_old_over_keyed": so["median_ms"] / sn["median_ms"],
            "keyed_sigs_per_s": n / (sn["median_ms"] * 1e-3), "old_sigs_per_s": n / (so["median_ms"] * 1e-3)}


def host_pair(engine, signer, seed, n, reps, warmup):
    rng = np.random.default_rng(n)
    arena = rng.integers(0, 256, n * MSG_LEN + 16, dtype=np.uint8)
    off = np.arange(n, dtype=np.uint64) * MSG_LEN
    ln = np.full(n, MSG_LEN, np.uint32)
    seeds = np.tile(np.frombuffer(seed, np.uint8), (n, 1))

    def clock(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    def old():
        return engine.sign_batch(seeds, arena, off, ln)[1]

    def keyed():
        return signer.sign(arena, off, ln)

    if not np.array_equal(old(), keyed()):
        raise SystemExit(f"n={n}: Signer.sign differs from Engine.sign_batch")
    for _ in range(warmup):
        old()
        keyed()
    t_old, t_new = [], []
    for _ in range(reps):
        t_old.append(clock(old))
        t_new.append(clock(keyed))
    so, sn = spread(t_old), spread(t_new)
    return {"n": n, "msg_len": MSG_LEN, "old": so, "keyed": sn, "ratio_old_over_keyed": so["median_ms"] / sn["median_ms"]}


def compiler_remarks():
    """cv_sign_keyed_kernel's registers, scratch and occupancy as the compiler reports them (device pass only, with
    the library's flags; needs hipcc, not a GPU)."""
    from corda_amd import build as B
    src = os.path.join(B.CSRC, "cv_k_sign.hip")
    cmd = [B.HIPCC] + B.CFLAGS + B.KERNEL_FLAGS + ["--offload-device-only", "-Rpass-analysis=kernel-resource-usage",
                                                  "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    block = text[text.index("cv_sign_keyed_kernel"):]
    grab = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))  # noqa: E731
    return {"kernel": "cv_sign_keyed_kernel", "vgprs": grab(" VGPRs"), "sgprs": grab("TotalSGPRs"),
            "scratch_bytes_per_lane": grab("ScratchSize [bytes/lane]"), "occupancy_waves_per_simd":
            grab("Occupancy [waves/SIMD]"), "source": "hipcc -Rpass-analysis=kernel-resource-usage"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sign_keyed.json"))
    ap.add_argument("--compiler-remarks", action="store_true",
                    help="only (re)write the record's kernel_resources from a compile of cv_k_sign.hip; no GPU needed")
    a = ap.parse_args()
    old = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
    if a.compiler_remarks:
        old["kernel_resources"] = compiler_remarks()
        with open(a.out, "w") as f:
            json.dump(old, f, indent=1)
            f.write("\n")
        print(old["kernel_resources"])
        return
    if a.reps < 20:
        raise SystemExit("at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("sign_bench needs a GPU")
    seed = bytes([20]) + bytes(31)                   # entropyToKeyPair(20), DUMMY_NOTARY_KEY
    engine = native.Engine(1)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    with native.Signer(engine, seed) as signer:
        rec = {"tool": "tools/sign_bench.py", "device": torch.cuda.get_device_name(0), "timer_device": "HIP events",
               "timer_host": "perf_counter around the synchronous call",
               "device_resident": [device_pair(engine, signer, seed, n, a.reps, a.warmup, stream) for n in SIZES],
               "device_resident_throughput": [device_pair(engine, signer, seed, THROUGHPUT_SIZE, a.reps, a.warmup,
                                                          stream)],
               "host_buffers": [host_pair(engine, signer, seed, n, a.reps, a.warmup) for n in SIZES]}
    engine.close()
    if "kernel_resources" in old:                    # kept from an earlier --compiler-remarks run
        rec["kernel_resources"] = old["kernel_resources"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for kind in ("device_resident", "device_resident_throughput", "host_buffers"):
        for r in rec[kind]:
            print(f"{kind:26s} n={r['n']:7d}  old {r['old']['median_ms']:.4f} ms  keyed {r['keyed']['median_ms']:.4f} ms"
                  f"  ratio {r['ratio_old_over_keyed']:.2f}", flush=True)


if __name__ == "__main__":
    main()
