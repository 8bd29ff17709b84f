#!/usr/bin/env python3
"""What building tear-offs on the GPU costs beside the Merkle ids of the same leaves.

C3 leaf shape (corda_amd/workload.py LEAF_SHAPE: 6 leaves per transaction, 2x120, 2x600, 2x300 bytes +-25 %) with 2
of the 6 kept (the first output and the first command), at 4,096 and 262,144 transactions, from host buffers:
  ids     cv_merkle_tx_ids_ex      leaf hashes + roots, the levels thrown away
  build   cv_filtered_build        leaf hashes + every level kept + the pruned trees emitted and copied back
both synchronous, timed with the host clock around the C call with the outputs allocated (and touched) beforehand,
the two calls alternating, `reps` repetitions each after a warm-up of both; median and interquartile range.  The
difference is what keeping the pyramid and emitting costs.  At 4,096 also the Python mirror's
FilteredTransaction.build_merkle_transaction loop (hashlib + objects, one transaction after another).  Before
anything is timed the build's ids are compared with the id call's and its trees with the mirror's.
Writes one JSON record (default profiles/pmt_build.json).  Needs a GPU: no fallback.

    python tools/pmt_build_bench.py [--reps 20] [--out profiles/pmt_build.json]
"""
import argparse
import ctypes
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
from corda_amd.transactions import FilteredTransaction, WireTransaction  # noqa: E402
from corda_amd.workload import LEAF_SHAPE  # noqa: E402

SIZES = (4096, 262144)
KEPT = (2, 4)                       # leaf positions kept in every transaction: the first output, the first command


def spread(xs):
    xs = sorted(xs)
    q = statistics.quantiles(xs, n=4)
    return {"median_ms": statistics.median(xs), "min_ms": xs[0], "max_ms": xs[-1], "iqr_ms": q[2] - q[0], "reps": len(xs)}


def clock(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def make(ntx):
    rng = np.random.default_rng(ntx)
    nleaf = len(LEAF_SHAPE)
    lens = (np.tile(np.array(LEAF_SHAPE, np.float64), ntx) * (rng.random(ntx * nleaf) * 0.5 + 0.75)).astype(np.uint32)
    offs = np.zeros(ntx * nleaf, np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    arena = rng.integers(0, 256, int(offs[-1]) + int(lens[-1]) + 16, dtype=np.uint8)
    begin = np.arange(0, ntx * nleaf + 1, nleaf, dtype=np.uint32)
    keep = np.zeros(ntx * nleaf, np.uint8)
    for k in KEPT:
        keep[k::nleaf] = 1
    return arena, offs, lens, begin, keep


def mirror_loop(arena, offs, lens, ntx):
    nleaf = len(LEAF_SHAPE)
    blob = lambda i: arena[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes()  # noqa: E731
    wtxs = [WireTransaction(inputs=[blob(t * nleaf), blob(t * nleaf + 1)], outputs=[blob(t * nleaf + 2), blob(t * nleaf + 3)],
                            commands=[blob(t * nleaf + 4), blob(t * nleaf + 5)]) for t in range(ntx)]
    first_out = lambda w: (lambda b: b == w.outputs[0])  # noqa: E731
    first_cmd = lambda w: (lambda b: b == w.commands[0])  # noqa: E731

    def run():
        return [FilteredTransaction.build_merkle_transaction(w, filter_outputs=first_out(w), filter_commands=first_cmd(w))
                for w in wtxs]
    return run


def one_size(engine, ntx, reps, warmup):
    arena, offs, lens, begin, keep = make(ntx)
    lib, h, p = engine._lib, engine._h, native._p
    cap = native.partial_merkle_build_bound(begin)
    kind, left, right = np.ones(cap, np.uint8), np.ones(cap, np.uint32), np.ones(cap, np.uint32)
    hashes, tb = np.ones((cap, 32), np.uint8), np.ones(ntx + 1, np.uint32)
    ids_b, st_b, ids_i, st_i = (np.ones((ntx, 32), np.uint8), np.ones(ntx, np.uint8), np.ones((ntx, 32), np.uint8),
                                np.ones(ntx, np.uint8))
    nn = ctypes.c_size_t(0)

    def ids():
        rc = lib.cv_merkle_tx_ids_ex(h, ntx, p(arena), p(offs), p(lens), p(begin), p(ids_i), p(st_i))
        assert rc == 0, rc

    def build():
        rc = lib.cv_filtered_build(h, ntx, p(arena), arena.size, p(offs), p(lens), p(begin), p(keep), cap, p(kind), p(left),
                                   p(right), p(hashes), p(tb), p(ids_b), p(st_b), ctypes.byref(nn))
        assert rc == 0, rc

    ids()
    build()
    if not (np.array_equal(ids_b, ids_i) and not st_b.any() and not st_i.any()):
        raise SystemExit(f"ntx={ntx}: cv_filtered_build's ids differ from cv_merkle_tx_ids_ex's")
    rec = {"ntx": ntx, "leaves_per_tx": len(LEAF_SHAPE), "kept_per_tx": len(KEPT), "leaf_bytes": int(arena.size - 16),
           "nodes": int(nn.value), "nodes_per_tx": nn.value / ntx, "bound_nodes": int(cap)}
    run_mirror = None
    if ntx <= 4096:
        run_mirror = mirror_loop(arena, offs, lens, ntx)
        host = run_mirror()
        for t in range(ntx):
            k, l, r, hs = host[t].partial_merkle_tree.flatten(int(tb[t]))
            b, e = int(tb[t]), int(tb[t + 1])
            if not (k == kind[b:e].tolist() and l == left[b:e].tolist() and r == right[b:e].tolist()
                    and b"".join(hs) == hashes[b:e].tobytes()):
                raise SystemExit(f"ntx={ntx}: tree {t} differs from the mirror's")
    for _ in range(warmup):
        ids()
        build()
    t_ids, t_build = [], []
    for _ in range(reps):                            # interleaved: drift hits both alike
        t_ids.append(clock(ids))
        t_build.append(clock(build))
    rec["ids"], rec["build"] = spread(t_ids), spread(t_build)
    rec["build_minus_ids_ms"] = rec["build"]["median_ms"] - rec["ids"]["median_ms"]
    rec["build_over_ids"] = rec["build"]["median_ms"] / rec["ids"]["median_ms"]
    rec["build_tx_per_s"] = ntx / (rec["build"]["median_ms"] * 1e-3)
    if run_mirror:
        run_mirror()
        rec["python_mirror"] = spread([clock(run_mirror) for _ in range(reps)])
        rec["mirror_over_build"] = rec["python_mirror"]["median_ms"] / rec["build"]["median_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pmt_build.json"))
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("pmt_build_bench needs a GPU")
    engine = native.Engine(1)
    rec = {"tool": "tools/pmt_build_bench.py", "device": torch.cuda.get_device_name(0),
           "timer": "perf_counter around the synchronous C call, host buffers (pageable), outputs preallocated",
           "sizes": []}
    for n in SIZES:
        rec["sizes"].append(one_size(engine, n, a.reps, a.warmup))
        r = rec["sizes"][-1]
        print(f"ntx={n:7d}  ids {r['ids']['median_ms']:.3f} ms (iqr {r['ids']['iqr_ms']:.3f})  build "
              f"{r['build']['median_ms']:.3f} ms (iqr {r['build']['iqr_ms']:.3f})  nodes/tx {r['nodes_per_tx']:.2f}"
              + (f"  mirror {r['python_mirror']['median_ms']:.1f} ms" if "python_mirror" in r else ""), flush=True)
    engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
