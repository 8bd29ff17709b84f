#!/usr/bin/env python3
"""What an oracle's signing step costs end to end from host buffers: the composition a binding had before
cv_tearoff_sign_batch (A: the filtered hashes with hashlib on the host, cv_partial_merkle_verify, the gate in numpy,
cv_ed25519_sign_keyed over the accepted roots) against the one fused call (B), DESIGN.md §5.12.

Shape: ntx tear-offs (256, 4,096 and 65,536) of 6-leaf transactions (workload.LEAF_SHAPE: 2 inputs, 2 outputs, 2
commands) with the 2 commands kept; the trees come from cv_filtered_build, the verifier's arena holds the kept leaves
alone.  Every 16th tear-off is refused, cycling through a wrong root and a leaf_pre of 1, 2 and 3.  A and B run
interleaved in one process, one repetition after the other on the same batch, the order alternating; their outcomes,
first_bad and signatures are compared in every repetition.  Timed with the host clock around the synchronous calls,
inputs prepared and outputs allocated by the binding inside the timed span for both.  A's C calls are also summed on
their own (`a_calls_only`): the difference to `a` is its hashlib / numpy glue.  Reports p50 and p99.
Writes one JSON record (default profiles/tearoff_fused.json).  Needs a GPU: no fallback.

    python tools/tearoff_bench.py [--reps 200] [--out profiles/tearoff_fused.json]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from corda_amd import native, workload  # noqa: E402

LEAVES, KEPT = len(workload.LEAF_SHAPE), 2
SIZES = (256, 4096, 65536)
NO_LEAF = native.TS_NO_LEAF


def make(engine, ntx, seed):
    rng = np.random.default_rng(seed)
    lens = (np.tile(np.array(workload.LEAF_SHAPE), ntx) * (rng.random(ntx * LEAVES) * 0.5 + 0.75)).astype(np.uint32)
    offs = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
    arena = np.frombuffer(rng.bytes(int(lens.sum()) + 16), np.uint8)
    begin = np.arange(0, ntx * LEAVES + 1, LEAVES, dtype=np.uint32)
    keep = np.tile(np.array([0] * (LEAVES - KEPT) + [1] * KEPT, np.uint8), ntx)
    kind, left, right, hashes, tb, ids, st = engine.filtered_build(arena, offs, lens, begin, keep)
    if st.any():
        raise SystemExit("cv_filtered_build refused a transaction of the batch")
    # the verifier's side: the kept leaves alone, in an arena of their own
    kept = np.flatnonzero(keep)
    blobs = [arena[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs[kept], lens[kept])]
    klen = lens[kept]
    koff = (np.cumsum(klen, dtype=np.uint64) - klen).astype(np.uint64)
    root, pre = ids.copy(), np.zeros(kept.size, np.uint8)
    for j, t in enumerate(range(seed % 16, ntx, 16)):
        if j % 4 == 0:
            root[t, j % 32] ^= 1
        else:
            pre[KEPT * t + j % KEPT] = j % 4
    return dict(ntx=ntx, arena=np.frombuffer(b"".join(blobs) + bytes(16), np.uint8), leaf_off=koff, leaf_len=klen,
                txb=np.arange(0, KEPT * ntx + 1, KEPT, dtype=np.uint32), kind=kind, left=left, right=right,
                node_hash=hashes, tree_begin=tb, root=root, pre=pre)


def run_a(engine, signer, b):
    """The composition -> (outcome, first_bad, sig, seconds inside the C calls)."""
    ntx, txb, pre = b["ntx"], b["txb"], b["pre"]
    a, off, ln = b["arena"], b["leaf_off"], b["leaf_len"]
    check = np.frombuffer(b"".join(hashlib.sha256(a[int(o):int(o) + int(n)]).digest() for o, n in zip(off, ln)), np.uint8)
    calls = 0.0
    t = time.perf_counter()
    v, st = engine.partial_merkle_verify(b["kind"], b["left"], b["right"], b["node_hash"], b["tree_begin"], b["root"],
                                         check.reshape(-1, 32), txb)
    calls += time.perf_counter() - t
    # the gate (NodeInterestRates.kt:190-217), vectorised; every tear-off of this shape has leaves
    idx = np.arange(pre.size, dtype=np.uint32)
    outcome = np.zeros(ntx, np.uint8)
    first_bad = np.full(ntx, NO_LEAF, np.uint32)
    for cls in (3, 2, 1):
        first = np.minimum.reduceat(np.where(pre == cls, idx, NO_LEAF), txb[:-1])
        hit = first != NO_LEAF
        outcome[hit], first_bad[hit] = native.CV_TS_VERIFY_FAILED + cls, first[hit]
    early = (st != 0) | (v == 0)
    outcome[early] = np.where(st[early] != 0, native.CV_TS_MALFORMED, native.CV_TS_VERIFY_FAILED)
    first_bad[early] = NO_LEAF
    acc = np.flatnonzero(outcome == 0)
    sig = np.zeros((ntx, 64), np.uint8)
    t = time.perf_counter()
    if acc.size:
        sig[acc] = signer.sign(b["root"].reshape(-1), (acc * 32).astype(np.uint64), np.full(acc.size, 32, np.uint32))
    calls += time.perf_counter() - t
    return outcome, first_bad, sig, calls


def run_b(engine, signer, b):
    return engine.tearoff_sign_batch(signer, b["arena"], b["leaf_off"], b["leaf_len"], b["txb"], b["kind"], b["left"],
                                     b["right"], b["node_hash"], b["tree_begin"], b["root"], b["pre"])


def pct(xs):
    xs = np.sort(np.array(xs)) * 1e3
    return {"p50_ms": float(np.percentile(xs, 50)), "p99_ms": float(np.percentile(xs, 99)), "min_ms": float(xs[0]),
            "reps": int(xs.size)}


def one_size(engine, signer, ntx, reps):
    b = make(engine, ntx, 1000 * ntx + 5)
    run_a(engine, signer, b)                                       # untimed: the workspaces grow here
    run_b(engine, signer, b)
    ta, tb, tac = [], [], []
    accepted = None
    for rep in range(reps):
        order = (0, 1) if rep % 2 == 0 else (1, 0)                 # alternate who goes first
        res = {}
        for which in order:
            t = time.perf_counter()
            res[which] = run_a(engine, signer, b) if which == 0 else run_b(engine, signer, b)
            (ta if which == 0 else tb).append(time.perf_counter() - t)
        tac.append(res[0][3])
        if not all(np.array_equal(x, y) for x, y in zip(res[0][:3], res[1])):
            raise SystemExit(f"ntx={ntx} rep {rep}: the fused call and the composition disagree")
        accepted = int((res[1][0] == 0).sum())
    rec = {"ntx": ntx, "leaves": LEAVES, "kept": KEPT, "accepted": accepted, "a_composition": pct(ta),
           "a_calls_only": pct(tac), "b_fused": pct(tb)}
    rec["a_over_b_p50"] = rec["a_composition"]["p50_ms"] / rec["b_fused"]["p50_ms"]
    rec["a_calls_only_over_b_p50"] = rec["a_calls_only"]["p50_ms"] / rec["b_fused"]["p50_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tearoff_fused.json"))
    a = ap.parse_args()
    if a.reps < 50:
        raise SystemExit("at least 50 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("tearoff_bench needs a GPU")
    engine = native.Engine(1)
    signer = native.Signer(engine, bytes(range(32)))
    rec = {"tool": "tools/tearoff_bench.py", "device": torch.cuda.get_device_name(0),
           "timer": "perf_counter around the synchronous calls through the ctypes binding, host buffers (pageable); A and B "
                    "interleaved per repetition on the same batch, the order alternating",
           "margin": "the fused p50 may exceed the composition's by the 5 % box-to-box spread of DESIGN.md at the most",
           "sizes": []}
    ok = True
    for n in a.sizes:
        r = one_size(engine, signer, n, a.reps)
        rec["sizes"].append(r)
        ok &= r["b_fused"]["p50_ms"] <= 1.05 * r["a_composition"]["p50_ms"]
        print(f"ntx={n:6d}  A composition p50 {r['a_composition']['p50_ms']:.3f} p99 {r['a_composition']['p99_ms']:.3f} ms "
              f"(C calls alone p50 {r['a_calls_only']['p50_ms']:.3f})  B fused p50 {r['b_fused']['p50_ms']:.3f} p99 "
              f"{r['b_fused']['p99_ms']:.3f} ms  A/B {r['a_over_b_p50']:.2f}", flush=True)
    rec["b_p50_within_5_percent_of_a_everywhere"] = bool(ok)
    signer.close()
    engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    if not ok:
        raise SystemExit("the fused call's p50 is more than 5 % above the composition's at some size")


if __name__ == "__main__":
    main()
