#!/usr/bin/env python3
"""What the hot-key route (cv_ed25519_verify_device_hotkeys) costs and saves against the unkeyed
device call on the same inputs, resident in HBM.  Shapes, 300-byte messages (the C2 shape):
  (a) half of the signatures under 64 keys, half under keys of their own — at 1M, 65,536 and 10,000 signatures;
  (b) 1M signatures, all keys distinct: the route finds nothing hot, so this is its overhead;
  (c) 1M signatures under a pool of 1,024 keys: everything is hot — also against cv_ed25519_dedupe_keys_device +
      cv_ed25519_verify_device_keyed.
Forms per shape, alternating in one process, each timed with HIP events around the entry point on one stream, --reps
repetitions after --warmup warm-ups: `unkeyed` cv_ed25519_verify_device; `hotkeys` the route (hot_min 8); `front` the
route with hot_min = n + 1 (the dedupe, tally, classification, record scan and read-back, then the unkeyed verify over
the caller's arrays: front - unkeyed is what the route costs before it decides); `dedupe` the device dedupe alone;
(c) `dedupe+keyed`.  Every form's verdicts are compared with the expected ones (one signature in 16 corrupted) before
timing.  Median and interquartile range in ms; one JSON record (default profiles/hotkeys.json).  Needs a GPU: no fallback.

    python tools/hotkeys_bench.py [--reps 20] [--warmup 5] [--out profiles/hotkeys.json] [--max-n 1048576]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from corda_amd import native  # noqa: E402

DEV = "cuda:0"
MSG = 300


def make(engine, n, shape, seed):
    """-> device arrays and the expected verdicts.  who[i]: the signer of record i."""
    rng = np.random.default_rng(seed)
    if shape == "a":
        who = np.where(rng.integers(0, 2, n) == 0, rng.integers(0, 64, n), 64 + np.arange(n))
    elif shape == "b":
        who = np.arange(n)
    else:
        who = rng.integers(0, 1024, n)
    ids, inv = np.unique(who, return_inverse=True)
    seeds = rng.integers(0, 256, (len(ids), 32), dtype=np.uint8)[inv]
    arena = rng.integers(0, 256, n * MSG, dtype=np.uint8)
    off = np.arange(n, dtype=np.uint64) * MSG
    ln = np.full(n, MSG, np.uint32)
    pk, sig = engine.sign_batch(seeds, arena, off, ln)
    bad = np.arange(n) % 16 == 5
    sig[bad, 9] ^= 4
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(n=n, pk=up(pk), sig=up(sig), arena=up(arena), off=up(off.view(np.int64)), len=up(ln.view(np.int32)),
                want=~bad, nkeys=len(ids))


def quartiles(ms):
    q1, q2, q3 = np.percentile(ms, [25, 50, 75])
    return dict(median_ms=round(float(q2), 4), iqr_ms=round(float(q3 - q1), 4))


def run_shape(engine, b, name, reps, warmup):
    n = b["n"]
    words = (n + 63) // 64
    ts = torch.cuda.Stream()                                 # a stream of the run's own: the engine takes it by handle
    stream = ts.cuda_stream
    bm = torch.zeros(words, dtype=torch.int64, device=DEV)
    ws = torch.empty(native.verify_hotkeys_workspace(n), dtype=torch.uint8, device=DEV)
    dws = torch.empty(native.dedupe_keys_workspace(n), dtype=torch.uint8, device=DEV)
    keys = torch.empty(32 * n, dtype=torch.uint8, device=DEV)
    kidx = torch.empty(n, dtype=torch.int32, device=DEV)
    nk = torch.empty(4, dtype=torch.int32, device=DEV)
    P = lambda t: t.data_ptr()
    args = (P(b["pk"]), P(b["sig"]), P(b["arena"]), P(b["off"]), P(b["len"]), P(bm))
    route = {}

    def unkeyed():
        engine.verify_device(0, n, *args, 0, stream)

    def hotkeys():
        route["hotkeys"] = engine.verify_device_hotkeys(0, n, *args, 0, P(ws), hot_min=0, stream=stream)

    def front():
        route["front"] = engine.verify_device_hotkeys(0, n, *args, 0, P(ws), hot_min=n + 1, stream=stream)

    def dedupe():
        engine.dedupe_keys_device(0, n, P(b["pk"]), P(keys), P(kidx), P(nk), P(dws), stream)

    def dedupe_keyed():
        dedupe()
        ts.synchronize()
        engine.verify_device_keyed(0, n, int(nk[0].item()), P(keys), P(kidx), *args[1:], 0, stream)

    forms = {"unkeyed": unkeyed, "hotkeys": hotkeys, "front": front, "dedupe": dedupe}
    if name.startswith("c"):
        forms["dedupe+keyed"] = dedupe_keyed
    for f, fn in forms.items():                              # every form's verdicts before any timing
        if f == "dedupe":
            continue
        bm.fill_(-1)
        torch.cuda.synchronize()
        fn()
        torch.cuda.synchronize()
        got = native.bitmap_to_bools(bm.cpu().numpy().view(np.uint64), n)
        assert np.array_equal(got, b["want"]), (name, f)
    times = {f: [] for f in forms}
    for r in range(warmup + reps):
        for f, fn in forms.items():                          # the forms alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            fn()
            e1.record(ts)
            e1.synchronize()
            if r >= warmup:
                times[f].append(e0.elapsed_time(e1))
    rec = dict(shape=name, n=n, nkeys=b["nkeys"], route=route.get("hotkeys"), forms={f: quartiles(t) for f, t in times.items()})
    u, h = rec["forms"]["unkeyed"], rec["forms"]["hotkeys"]
    rec["hotkeys_over_unkeyed"] = round(h["median_ms"] / u["median_ms"], 3)
    rec["worth_setting"] = bool(h["median_ms"] < u["median_ms"] - u["iqr_ms"])
    rec["front_cost_ms"] = round(rec["forms"]["front"]["median_ms"] - u["median_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hotkeys.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    engine = native.Engine(1)
    engine.key_cache_reserve(2048)
    big = min(a.max_n, 1 << 20)
    out = []
    for name, shape, n in (("a_1M", "a", big), ("a_65536", "a", 65536), ("a_10000", "a", 10000), ("b_1M", "b", big),
                           ("c_1M", "c", big)):
        b = make(engine, n, shape, 20261021 + n)
        rec = run_shape(engine, b, name, a.reps, a.warmup)
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del b
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/hotkeys_bench.py", reps=a.reps, warmup=a.warmup, msg_bytes=MSG, shapes=out), f, indent=1)
        f.write("\n")
    engine.close()


if __name__ == "__main__":
    main()
