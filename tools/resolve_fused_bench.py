#!/usr/bin/env python3
"""What resolving a downloaded dependency chain costs end to end from host buffers, DESIGN.md §5.13:
  (a) the one fused call, cv_resolve_batch (Engine.resolve_batch);
  (b) the three component C calls it fuses, alone — cv_merkle_tx_ids, cv_ed25519_verify_batch over the ids,
      cv_missing_signers — with no graph work at all (no join, no duplicate check, no order, no walk);
  (c) the full composition, resolve.resolve_transactions(fused=False): those calls plus the Python restatement of the
      graph work over the transaction objects (what a binding had before the call), and for scale
  (a') resolve.resolve_transactions(fused=True), the fused call from the same objects.

Shape: bench.py's resolve chain — ntx transactions of 6 leaves (one input, two outputs, three commands) and 2 signers,
each spending output 0 of its predecessor, in download order (the newest first), one transaction in 16 with a flipped
signature bit (so the walk stops at the first of them; every transaction is still hashed, verified and joined).
Sizes 256, 5,000 (the flow's transactionCountLimit) and 65,536.  All variants run interleaved in one process, one
repetition after the other on the same batch, the order rotating; (a) and (b) are compared in every repetition
(outcomes against the component verdicts).  Timed with the host clock around the synchronous calls, inputs prepared
and outputs allocated by the binding inside the timed span.  The per-stage split of (a) comes from HIP events around the
stages of one further, untimed call (CV_OPT_TIMELINE, cv_diag_stats CV_STATS_RESOLVE).  Reports p50 and p99.
Acceptance at 5,000 transactions: p50(a) <= 1.10 x p50(b).  Writes one JSON record (default
profiles/resolve_fused.json).  Needs a GPU: no fallback.

    python tools/resolve_fused_bench.py [--reps 200] [--out profiles/resolve_fused.json]
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
from corda_amd import native, resolve  # noqa: E402
from corda_amd.crypto import DigitalSignature, KeyPair  # noqa: E402
from corda_amd.transactions import SecureHash, SignedTransaction, WireTransaction  # noqa: E402

SIZES = (256, 5000, 65536)
ACCEPT_AT, ACCEPT = 5000, 1.10
LEAVES, SIGNERS = 6, 2


def host_id(leaves) -> bytes:
    """WireTransaction.id on the host (MerkleTransaction.kt:66-99: the last hash of an odd level is duplicated)."""
    lvl = [hashlib.sha256(b).digest() for b in leaves]
    while len(lvl) > 1:
        if len(lvl) % 2:
            lvl.append(lvl[-1])
        lvl = [hashlib.sha256(lvl[i] + lvl[i + 1]).digest() for i in range(0, len(lvl), 2)]
    return lvl[0]


def make_chain(keys, ntx, seed):
    """-> the downloads, the newest first.  Built oldest first: an input names its predecessor's id."""
    rng = np.random.default_rng(seed)
    prev = SecureHash(hashlib.sha256(b"genesis %d" % seed).digest())
    must = [k.public.composite for k in keys]
    wtxs = []
    for t in range(ntx):
        blob = lambda tag: bytes(rng.integers(0, 256, int(rng.integers(40, 200)), dtype=np.uint8)) + tag
        w = WireTransaction(inputs=[resolve.StateRef(prev, 0).blob], outputs=[blob(b"o0"), blob(b"o1")],
                            commands=[blob(b"c0"), blob(b"c1"), blob(b"c2")], must_sign=must)
        w._id = prev = SecureHash(host_id(w.leaves))
        wtxs.append(w)
    sigs = [k.sign_many([w._id.bytes for w in wtxs]) for k in keys]
    stxs = []
    for t, w in enumerate(wtxs):
        mine = [s[t] for s in sigs]
        if t % 16 == seed % 16:
            bad = bytearray(mine[0].bits)
            bad[40] ^= 1
            mine[0] = DigitalSignature.WithKey(mine[0].by, bytes(bad))
        stxs.append(SignedTransaction(w, mine, w._id))
    return stxs[::-1]


def run_b(engine, args):
    pk, sig, tsb, _ = args["sigs"]
    ids, mst = engine.merkle_tx_ids(args["arena"], args["leaf_off"], args["leaf_len"], args["tx_leaf_begin"])
    nsig = int(tsb[-1])
    bm, sst = engine.verify_batch(pk, sig, ids.reshape(-1), (np.arange(nsig, dtype=np.uint64) // SIGNERS) * 32,
                                  np.full(nsig, 32, np.uint32))
    _, ck = engine.missing_signers(*args["reqs"], tsb, bitmap=bm)
    return native.tx_verdicts(bm, tsb).astype(bool) & (mst == 0) & (ck == 0)


def pct(xs):
    xs = np.sort(np.array(xs)) * 1e3
    return {"p50_ms": float(np.percentile(xs, 50)), "p99_ms": float(np.percentile(xs, 99)), "min_ms": float(xs[0]),
            "reps": int(xs.size)}


def one_size(engine, keys, ntx, reps):
    stxs = make_chain(keys, ntx, 7000 + ntx)
    args, _ = resolve.flatten_resolve(stxs)
    slow = max(10, reps // 10) if ntx > 10000 else reps            # the object paths at the largest size
    t = {k: [] for k in "abcm"}
    for w in range(3):                                             # warm-up: buffers grown, nothing timed
        engine.resolve_batch(**args)
        run_b(engine, args)
    want = resolve.resolve_transactions(stxs, engine, fused=False)
    got = resolve.resolve_transactions(stxs, engine, fused=True)
    if [s.id for s in want[0]] != [s.id for s in got[0]] or want[1] != got[1] or type(want[2]) is not type(got[2]):
        raise SystemExit(f"ntx={ntx}: the fused call and the composition disagree")
    for rep in range(reps):
        which = "abcm" if rep < slow else "ab"
        k0 = rep % len(which)
        for k in which[k0:] + which[:k0]:                          # rotate who goes first
            if k == "c":                                           # the composition hashes the ids again, as (a) does
                for s in stxs:
                    s._wtx._id, s._checked = None, False
            t0 = time.perf_counter()
            if k == "a":
                out = engine.resolve_batch(**args)
            elif k == "b":
                ok = run_b(engine, args)
            elif k == "c":
                resolve.resolve_transactions(stxs, engine, fused=False)
            else:
                resolve.resolve_transactions(stxs, engine, fused=True)
            t[k].append(time.perf_counter() - t0)
        if not np.array_equal(out["outcome"] == native.CV_RS_OK, ok):
            raise SystemExit(f"ntx={ntx} rep {rep}: the fused call and the component calls disagree")
    engine.set_option("timeline", 1)
    engine.stats("resolve", reset=True)
    engine.resolve_batch(**args)
    stages = engine.stats("resolve", reset=True)
    engine.set_option("timeline", 0)
    g = dict(zip(native.RG_WORDS, (int(v) for v in out["graph"])))
    rec = {"ntx": ntx, "signatures": ntx * SIGNERS, "leaves": LEAVES, "signers": SIGNERS, "inputs": int(len(args["input_index"])),
           "n_pass": g["n_pass"], "stop_class": g["stop_class"], "table_maxprobe": g["maxprobe"],
           "a_fused": pct(t["a"]), "b_component_calls": pct(t["b"]), "c_composition": pct(t["c"]),
           "a_mirror_fused": pct(t["m"]), "a_stages_ms": {k: round(v, 4) for k, v in stages.items() if k != "calls"}}
    rec["a_over_b_p50"] = rec["a_fused"]["p50_ms"] / rec["b_component_calls"]["p50_ms"]
    rec["c_over_a_p50"] = rec["c_composition"]["p50_ms"] / rec["a_fused"]["p50_ms"]
    rec["c_over_mirror_fused_p50"] = rec["c_composition"]["p50_ms"] / rec["a_mirror_fused"]["p50_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resolve_fused.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resolve_fused_bench needs a GPU")
    engine = native.Engine(1)
    keys = [KeyPair(hashlib.sha256(b"resolve bench key %d" % k).digest(), engine) for k in range(SIGNERS)]
    rec = {"tool": "tools/resolve_fused_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "timer": "perf_counter around the synchronous calls through the ctypes binding, host buffers (pageable); the "
                    "variants interleaved per repetition on the same batch, the order rotating; stages: HIP events around "
                    "the stages of one untimed call",
           "sizes": []}
    ok = None
    for n in a.sizes:
        r = one_size(engine, keys, n, a.reps)
        rec["sizes"].append(r)
        if n == ACCEPT_AT:
            ok = r["a_over_b_p50"] <= ACCEPT
        print(f"ntx={n:6d}  (a) fused p50 {r['a_fused']['p50_ms']:.3f} p99 {r['a_fused']['p99_ms']:.3f} ms  (b) component calls "
              f"p50 {r['b_component_calls']['p50_ms']:.3f} p99 {r['b_component_calls']['p99_ms']:.3f} ms  (c) composition p50 "
              f"{r['c_composition']['p50_ms']:.3f} ms  mirror fused p50 {r['a_mirror_fused']['p50_ms']:.3f} ms  a/b "
              f"{r['a_over_b_p50']:.3f}  c/a {r['c_over_a_p50']:.1f}  stages {r['a_stages_ms']}", flush=True)
    rec["acceptance"] = {"at_ntx": ACCEPT_AT, "bound_a_over_b_p50": ACCEPT, "met": ok}
    for k in keys:
        k.close()
    engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    if ok is False:
        raise SystemExit("p50 of the fused call is above 1.10 x the component calls' at 5,000 transactions")


if __name__ == "__main__":
    main()
