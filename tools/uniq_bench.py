#!/usr/bin/env python3
"""What the notary's commit step costs on the device-resident uniqueness set.

cv_uniq_commit_batch from host buffers at 4,096 and 262,144 requests x 2 states each, keys uniformly random 32 bytes
(what SHA-256 outputs look like to the table), three shapes:
  free      no state occurs twice
  spend16   one request in 16 spends, as its first state, the LAST state of a random EARLIER request of the batch; that
            request may be such a double spend itself, and if it is rejected the later one is free again, so the
            decisions depend on each other several levels deep (a dependency k levels deep takes k + 1 rounds)
  resident  `free` into a set that already holds 2^24 states (loaded by cv_uniq_load in 2^20-key calls)
Every repetition commits fresh keys into the same set (the set grows by a batch per repetition; it is opened with
room for all of them, so no repetition rehashes).  Timed with the host clock around the synchronous C call with the
outputs allocated and touched beforehand, `reps` repetitions after `warmup`; median and interquartile range.  The
rounds and the serial tail's share come from cv_uniq_stats after every repetition; the spend16 shape runs with
max_rounds at its cap (64), so `rounds_max` is the smallest max_rounds at which it never reaches the serial tail.
At 4,096 also InMemoryUniquenessProvider.commit_batch on the same requests (a fresh provider per repetition), and
before anything is timed the device's statuses are compared with that provider's.
Writes one JSON record (default profiles/uniq_commit.json).  Needs a GPU: no fallback.

    python tools/uniq_bench.py [--reps 20] [--out profiles/uniq_commit.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from corda_amd import native  # noqa: E402
from corda_amd.transactions import SecureHash  # noqa: E402
from corda_amd.uniqueness import InMemoryUniquenessProvider  # noqa: E402

SIZES = (4096, 262144)
PER_TX = 2
RESIDENT = 1 << 24
LOAD_CHUNK = 1 << 20


def spread(xs):
    xs = sorted(xs)
    q = statistics.quantiles(xs, n=4)
    return {"median_ms": statistics.median(xs), "min_ms": xs[0], "max_ms": xs[-1], "iqr_ms": q[2] - q[0], "reps": len(xs)}


def make(rng, ntx, spend16):
    keys = rng.integers(0, 256, (ntx * PER_TX, 32), dtype=np.uint8)
    if spend16:
        t = np.flatnonzero(rng.random(ntx) < 1 / 16)
        t = t[t > 0]
        earlier = (rng.random(t.shape[0]) * t).astype(np.int64)           # uniform in [0, t)
        keys[t * PER_TX] = keys[earlier * PER_TX + 1]
    return dict(key=keys, begin=np.arange(0, ntx * PER_TX + 1, PER_TX, dtype=np.uint32),
                id=rng.integers(0, 256, (ntx, 32), dtype=np.uint8), caller=(np.arange(ntx) % 16).astype(np.uint32))


def oracle_requests(b):
    ntx = b["id"].shape[0]
    return [([b["key"][PER_TX * t + j].tobytes() for j in range(PER_TX)], SecureHash(b["id"][t].tobytes()), int(b["caller"][t]))
            for t in range(ntx)]


def one_shape(engine, ntx, shape, reps, warmup):
    rng = np.random.default_rng(ntx * 3 + len(shape))
    lib, p = engine._lib, native._p
    total = reps + warmup + 1
    preload = RESIDENT if shape == "resident" else 0
    s = native.UniquenessSet(engine, preload + total * ntx * PER_TX)
    for c in range(0, preload, LOAD_CHUNK):
        s.load(rng.integers(0, 256, (LOAD_CHUNK, 32), dtype=np.uint8), rng.integers(0, 256, (LOAD_CHUNK, 32), dtype=np.uint8),
               np.zeros(LOAD_CHUNK, np.uint32), np.zeros(LOAD_CHUNK, np.uint32))
    if shape == "spend16":
        s.set_max_rounds(64)
    ns = ntx * PER_TX
    out = (np.ones(ntx, np.uint8), np.ones(ns, np.uint8), np.ones((ns, 32), np.uint8), np.ones(ns, np.uint32),
           np.ones(ns, np.uint32))

    def commit(b):
        t = time.perf_counter()
        rc = lib.cv_uniq_commit_batch(s._h, ntx, p(b["key"]), p(b["begin"]), p(b["id"]), p(b["caller"]), None,
                                      *[p(a) for a in out])
        dt = (time.perf_counter() - t) * 1e3
        assert rc == 0, rc
        return dt

    # correctness first, against the provider the parent commit had (at 262,144 the loop takes a few seconds)
    b = make(rng, ntx, shape == "spend16")
    commit(b)
    want = InMemoryUniquenessProvider().commit_batch(oracle_requests(b))
    if [int(x) for x in out[0]] != [0 if w is None else 1 for w in want]:
        raise SystemExit(f"{shape} ntx={ntx}: statuses differ from InMemoryUniquenessProvider's")
    rec = {"ntx": ntx, "states_per_tx": PER_TX, "shape": shape, "resident_before": preload,
           "conflicts_first_batch": int((out[0] == 1).sum())}
    for _ in range(warmup):
        commit(make(rng, ntx, shape == "spend16"))
    times, rounds, tail, probe = [], [], [], []
    for _ in range(reps):
        times.append(commit(make(rng, ntx, shape == "spend16")))
        st = s.stats()
        rounds.append(st["rounds"])
        tail.append(st["tail"])
        probe.append(st["probe"])
    rec["commit"] = spread(times)
    rec["requests_per_s"] = ntx / (rec["commit"]["median_ms"] * 1e-3)
    rec.update(rounds_min=min(rounds), rounds_max=max(rounds), tail_max=max(tail), probe_max=max(probe),
               resident_after=s.stats()["resident"], slots=s.stats()["slots"])
    if ntx <= 4096 and shape != "resident":
        reqs = [oracle_requests(make(rng, ntx, shape == "spend16")) for _ in range(reps)]

        def host(r):
            prov = InMemoryUniquenessProvider()
            t = time.perf_counter()
            prov.commit_batch(r)
            return (time.perf_counter() - t) * 1e3
        host(reqs[0])
        rec["in_memory_provider"] = spread([host(r) for r in reqs])
        rec["in_memory_over_device"] = rec["in_memory_provider"]["median_ms"] / rec["commit"]["median_ms"]
    s.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "uniq_commit.json"))
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("uniq_bench needs a GPU")
    engine = native.Engine(1)
    rec = {"tool": "tools/uniq_bench.py", "device": torch.cuda.get_device_name(0),
           "timer": "perf_counter around the synchronous C call, host buffers (pageable), outputs preallocated; "
                    "upload, kernels and copy-back are not timed apart",
           "shapes": []}
    for n in SIZES:
        for shape in ("free", "spend16", "resident"):
            r = one_shape(engine, n, shape, a.reps, a.warmup)
            rec["shapes"].append(r)
            print(f"ntx={n:7d} {shape:9s} commit {r['commit']['median_ms']:.3f} ms (iqr {r['commit']['iqr_ms']:.3f})  rounds "
                  f"{r['rounds_min']}-{r['rounds_max']}  tail {r['tail_max']}  probe {r['probe_max']}"
                  + (f"  in-memory {r['in_memory_provider']['median_ms']:.2f} ms" if "in_memory_provider" in r else ""),
                  flush=True)
    engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
