#!/usr/bin/env python3
"""Many-key signing from the device key store against what a caller had before it.

Host-buffer calls (copies in, kernels, copies out, synchronous), one process, 32-byte messages, the host clock around
each call, at n = 4,096 / 65,536 / 1,048,576 signatures:
  store   cv_keystore_sign over a 1,024-key store, the key drawn per record
  seeds   cv_ed25519_sign_batch with the record's seed (a key expansion per signature): what a caller has without it
  keyed   cv_ed25519_sign_keyed with ONE key for every record: the floor
and, for n / 2 transactions of 6 leaves and 2 keys each:
  fused     cv_sign_transactions
  composed  cv_merkle_tx_ids_bounded, then cv_keystore_sign over the ids
The paths of a group alternate, `reps` repetitions each after a warm-up of all; median and spread (min, max,
interquartile range) per call.  The signatures of store and seeds, and of fused and composed, are compared byte for
byte at each size before anything is timed.  Writes one JSON record (default profiles/keystore.json).  Needs a GPU:
no fallback.

    python tools/keystore_bench.py [--reps 20] [--out profiles/keystore.json]
    python tools/keystore_bench.py --compiler-remarks     # adds the kernels' VGPRs / scratch / occupancy to the record
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from corda_amd import native  # noqa: E402

SIZES = (4096, 65536, 1 << 20)
STORE_KEYS = 1024
MSG_LEN = 32
TX_LEAVES, TX_KEYS, LEAF_LEN = 6, 2, 80


def spread(xs):
    xs = sorted(xs)
    q = statistics.quantiles(xs, n=4)
    return {"median_ms": statistics.median(xs), "min_ms": xs[0], "max_ms": xs[-1], "iqr_ms": q[2] - q[0],
            "reps": len(xs)}


def clock(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def alternate(paths, reps, warmup):
    """paths: {name: fn}; every repetition runs each path once, in order: drift hits all alike."""
    for _ in range(warmup):
        for fn in paths.values():
            fn()
    times = {k: [] for k in paths}
    for _ in range(reps):
        for k, fn in paths.items():
            times[k].append(clock(fn))
    return {k: spread(v) for k, v in times.items()}


def sign_group(engine, ks, signer, seeds, pks, n, reps, warmup):
    rng = np.random.default_rng(n)
    arena = rng.integers(0, 256, n * MSG_LEN + 16, dtype=np.uint8)
    off = np.arange(n, dtype=np.uint64) * MSG_LEN
    ln = np.full(n, MSG_LEN, np.uint32)
    which = rng.integers(0, STORE_KEYS, n)
    rec_seed, rec_pk = np.ascontiguousarray(seeds[which]), np.ascontiguousarray(pks[which])
    paths = {"store": lambda: ks.sign(rec_pk, arena, off, ln)[0],
             "seeds": lambda: engine.sign_batch(rec_seed, arena, off, ln)[1],
             "keyed": lambda: signer.sign(arena, off, ln)}
    if not np.array_equal(paths["store"](), paths["seeds"]()):
        raise SystemExit(f"n={n}: cv_keystore_sign differs from cv_ed25519_sign_batch with the record's seed")
    r = alternate(paths, reps, warmup)
    return {"n": n, "msg_len": MSG_LEN, "store_keys": STORE_KEYS, **r,
            "ratio_seeds_over_store": r["seeds"]["median_ms"] / r["store"]["median_ms"],
            "ratio_store_over_keyed": r["store"]["median_ms"] / r["keyed"]["median_ms"],
            "store_sigs_per_s": n / (r["store"]["median_ms"] * 1e-3)}


def tx_group(engine, ks, pks, nsig, reps, warmup):
    ntx = nsig // TX_KEYS
    rng = np.random.default_rng(nsig + 1)
    nl = ntx * TX_LEAVES
    arena = rng.integers(0, 256, nl * LEAF_LEN + 16, dtype=np.uint8)
    loff = np.arange(nl, dtype=np.uint64) * LEAF_LEN
    llen = np.full(nl, LEAF_LEN, np.uint32)
    lb = np.arange(ntx + 1, dtype=np.uint32) * TX_LEAVES
    sb = np.arange(ntx + 1, dtype=np.uint32) * TX_KEYS
    # two different keys a transaction
    first = rng.integers(0, STORE_KEYS, ntx)
    which = np.stack([first, (first + 1 + rng.integers(0, STORE_KEYS - 1, ntx)) % STORE_KEYS], axis=1).reshape(-1)
    pk = np.ascontiguousarray(pks[which])
    moff = np.repeat(np.arange(ntx, dtype=np.uint64) * 32, TX_KEYS)
    mlen = np.full(nsig, 32, np.uint32)

    def fused():
        return ks.sign_transactions(arena, loff, llen, lb, pk, sb)

    def composed():
        ids, _ = engine.merkle_tx_ids(arena, loff, llen, lb)
        return ks.sign(pk, ids.reshape(-1), moff, mlen)[0]

    st, _, sig, _ = fused()
    if st.any() or not np.array_equal(sig, composed()):
        raise SystemExit(f"nsig={nsig}: cv_sign_transactions differs from cv_merkle_tx_ids_bounded + cv_keystore_sign")
    r = alternate({"fused": fused, "composed": composed}, reps, warmup)
    return {"nsig": nsig, "ntx": ntx, "leaves_per_tx": TX_LEAVES, "keys_per_tx": TX_KEYS, "leaf_len": LEAF_LEN, **r,
            "ratio_composed_over_fused": r["composed"]["median_ms"] / r["fused"]["median_ms"]}


def compiler_remarks():
    """The key store's kernels' registers, scratch and occupancy as the compiler reports them (device pass only, with
    the library's flags; needs hipcc, not a GPU)."""
    from corda_amd import build as B
    src = os.path.join(B.CSRC, "cv_k_keystore.hip")
    cmd = [B.HIPCC] + B.CFLAGS + B.KERNEL_FLAGS + ["--offload-device-only", "-Rpass-analysis=kernel-resource-usage",
                                                  "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out = []
    for kernel in ("cv_ks_sign_kernel", "cv_ks_expand_kernel"):
        block = text[text.index(kernel):]
        grab = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))  # noqa: E731
        out.append({"kernel": kernel, "vgprs": grab(" VGPRs"), "sgprs": grab("TotalSGPRs"),
                    "scratch_bytes_per_lane": grab("ScratchSize [bytes/lane]"),
                    "occupancy_waves_per_simd": grab("Occupancy [waves/SIMD]"),
                    "source": "hipcc -Rpass-analysis=kernel-resource-usage"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "keystore.json"))
    ap.add_argument("--compiler-remarks", action="store_true",
                    help="only (re)write the record's kernel_resources from a compile of cv_k_keystore.hip; no GPU needed")
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
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("keystore_bench needs a GPU")
    engine = native.Engine(1)
    seeds = np.random.default_rng(1024).integers(0, 256, (STORE_KEYS, 32), dtype=np.uint8)
    with native.KeyStore(engine, STORE_KEYS) as ks, native.Signer(engine, seeds[0].tobytes()) as signer:
        pks, st = ks.add(seeds)
        if st.any():
            raise SystemExit("the bench's seeds repeat a key")
        rec = {"tool": "tools/keystore_bench.py", "device": torch.cuda.get_device_name(0),
               "timer": "perf_counter around the synchronous host-buffer call",
               "sign": [sign_group(engine, ks, signer, seeds, pks, n, a.reps, a.warmup) for n in SIZES],
               "transactions": [tx_group(engine, ks, pks, n, a.reps, a.warmup) for n in SIZES]}
    engine.close()
    if "kernel_resources" in old:                    # kept from an earlier --compiler-remarks run
        rec["kernel_resources"] = old["kernel_resources"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for r in rec["sign"]:
        print(f"sign n={r['n']:7d}  store {r['store']['median_ms']:.3f} ms  seeds {r['seeds']['median_ms']:.3f} ms  keyed "
              f"{r['keyed']['median_ms']:.3f} ms  seeds/store {r['ratio_seeds_over_store']:.2f}  store/keyed "
              f"{r['ratio_store_over_keyed']:.2f}", flush=True)
    for r in rec["transactions"]:
        print(f"txs  nsig={r['nsig']:7d}  fused {r['fused']['median_ms']:.3f} ms  composed {r['composed']['median_ms']:.3f} ms"
              f"  composed/fused {r['ratio_composed_over_fused']:.2f}", flush=True)


if __name__ == "__main__":
    main()
