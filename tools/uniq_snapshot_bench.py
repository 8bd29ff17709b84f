"""Snapshot and install of the device uniqueness set, measured (recorded, not gated): writes profiles/uniq_snapshot.json.

For sets of 2^16, 2^20 and 2^24 entries (--sizes), interleaved repetition by repetition in one process:
  snapshot_all     a full pass of cv_uniq_snapshot into pinned host buffers with max_entries = the resident count
  snapshot_64k     the same pass with max_entries = 2^16
  install          cv_uniq_install of that snapshot into a second set
  d2h_copy         the bound: hipMemcpy of 76 * n bytes from a device buffer into pinned host memory
  restart_log      the restart path without snapshots: DeviceUniquenessProvider(log=...) opened on a SQLite log of the
                   same number of entries (every row read and re-keyed in Python, then cv_uniq_load); fewer repetitions
                   where one takes seconds (--log-reps-large)
Each snapshot time is also reported as a multiple of the copy bound.  p50 over --reps repetitions (default 20).  The
restart's seconds of Python leave the device idle, so one untimed copy follows it before the timed calls.

    python tools/uniq_snapshot_bench.py [--sizes 16,20,24] [--reps 20] [--out profiles/uniq_snapshot.json]
"""
import argparse
import ctypes
import json
import os
import sqlite3
import struct
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from corda_amd import native  # noqa: E402
from corda_amd.uniqueness import DeviceUniquenessProvider, PersistentUniquenessProvider  # noqa: E402

DONE = 0xFFFFFFFFFFFFFFFF


def stats(ts):
    a = np.sort(np.asarray(ts)) * 1e3
    return {"p50_ms": round(float(np.percentile(a, 50)), 4), "p25_ms": round(float(np.percentile(a, 25)), 4),
            "p75_ms": round(float(np.percentile(a, 75)), 4), "min_ms": round(float(a[0]), 4), "reps": len(a)}


def entries(n, seed):
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    key[:, :8] = np.arange(n, dtype=np.uint64).view(np.uint8).reshape(n, 8)      # distinct by construction
    return key, rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 1 << 16, n, dtype=np.uint32), \
        rng.integers(0, 64, n, dtype=np.uint32)


def snapshot_pass(s, bufs, m):
    """One pass into the pinned buffers (the chunks of a chunked pass land behind one another) -> (seconds, calls)."""
    lib, h, p = s._lib, s._h, native._p
    cursor, n = np.zeros(2, np.uint64), ctypes.c_size_t(0)
    key, cid, cix, cc = bufs
    done = calls = 0
    t0 = time.perf_counter()
    while int(cursor[0]) != DONE:
        rc = lib.cv_uniq_snapshot(h, p(cursor), m, key[done:].ctypes.data, cid[done:].ctypes.data, cix[done:].ctypes.data,
                                  cc[done:].ctypes.data, ctypes.byref(n))
        if rc:
            raise native.CvError(rc, "cv_uniq_snapshot")
        done += n.value
        calls += 1
    return time.perf_counter() - t0, calls, done


def build_log(path, n):
    """A commit log of n rows, written with SQLite's durability off (building it is not what is measured)."""
    PersistentUniquenessProvider(path).close()
    db = sqlite3.connect(path, isolation_level=None)
    db.execute("PRAGMA synchronous=OFF")
    db.execute("BEGIN")
    tx = bytes(32)
    step = 1 << 16
    for b in range(0, n, step):
        db.executemany(f"INSERT INTO {PersistentUniquenessProvider.TABLE} VALUES (?, ?, ?, ?)",
                       ((b"B" + struct.pack("<I", 32) + struct.pack("<Q", i) + tx[:24], tx, i & 3, f"party-{i & 63}")
                        for i in range(b, min(b + step, n))))
    db.execute("COMMIT")
    db.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20,24", help="log2 of the entry counts")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log-reps-large", type=int, default=2, help="restart repetitions from 2^22 entries up")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "uniq_snapshot.json"))
    a = ap.parse_args()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    engine = native.Engine(0)
    runs = []
    for lg in (int(x) for x in a.sizes.split(",")):
        n = 1 << lg
        e = entries(n, lg)
        src, dst = native.UniquenessSet(engine, n), native.UniquenessSet(engine, 16)
        src.load(*e)
        bufs = (engine.host_empty((n, 32)), engine.host_empty((n, 32)), engine.host_empty(n, np.uint32),
                engine.host_empty(n, np.uint32))
        flat = engine.host_empty(76 * n)
        dbuf = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(dbuf), 76 * n) == 0
        tmp = tempfile.mkdtemp(prefix="uniq_snapshot_bench_")
        log_path = os.path.join(tmp, "log.db")
        build_log(log_path, n)
        t = {k: [] for k in ("snapshot_all", "snapshot_64k", "install", "d2h_copy", "restart_log")}
        calls = {}
        def copy():
            t0 = time.perf_counter()
            assert hip.hipMemcpy(flat.ctypes.data, dbuf, 76 * n, 2) == 0
            return time.perf_counter() - t0

        for rep in range(a.reps + 1):                 # the first repetition warms the workspace and is dropped
            if rep < (a.reps + 1 if lg < 22 else a.log_reps_large):
                log = PersistentUniquenessProvider(log_path)
                t0 = time.perf_counter()
                prov = DeviceUniquenessProvider(engine, capacity=n, log=log)
                t["restart_log"].append(time.perf_counter() - t0)
                assert len(prov) == n
                prov.close()
                log.close()
            copy()                                    # untimed: the device has idled for as long as the restart's Python ran
            dt, calls["snapshot_all"], got = snapshot_pass(src, bufs, n)
            assert got == n
            t["snapshot_all"].append(dt)
            t["d2h_copy"].append(copy())
            dt, calls["snapshot_64k"], got = snapshot_pass(src, bufs, 1 << 16)
            assert got == n
            t["snapshot_64k"].append(dt)
            t0 = time.perf_counter()
            dst.install(*bufs)
            t["install"].append(time.perf_counter() - t0)
        assert dst.stats()["resident"] == n
        drop = {k: (v[1:] if k != "restart_log" or lg < 22 else v) for k, v in t.items()}
        run = {"entries": n, "slots": src.stats()["slots"], "bytes_76n": 76 * n, "calls": calls}
        run.update({k: stats(v) for k, v in drop.items()})
        bound = run["d2h_copy"]["p50_ms"]
        run["snapshot_all_over_copy"] = round(run["snapshot_all"]["p50_ms"] / bound, 3)
        run["snapshot_64k_over_copy"] = round(run["snapshot_64k"]["p50_ms"] / bound, 3)
        run["copy_GBps"] = round(76 * n / bound / 1e6, 2)
        run["restart_over_snapshot_install"] = round(run["restart_log"]["p50_ms"] /
                                                     (run["snapshot_all"]["p50_ms"] + run["install"]["p50_ms"]), 1)
        runs.append(run)
        print(json.dumps(run), flush=True)
        hip.hipFree(dbuf)
        src.close()
        dst.close()
        del bufs, flat
        os.remove(log_path)
    out = {"what": "cv_uniq_snapshot / cv_uniq_install against the plain device-to-host copy of 76 * n bytes (the bound) "
                   "and against the restart from a SQLite commit log, one MI355X, one process, interleaved; times in ms, "
                   "pinned host buffers; p50 over the repetitions after one warm-up",
           "tool": "tools/uniq_snapshot_bench.py", "runs": runs}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    engine.close()


if __name__ == "__main__":
    main()
