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

--key-pool K draws each transaction's two signers from K keys instead of the chain's two parties; --fused-keyed {0,1,2}
sets CV_OPT_FUSED_KEYED for the run (0 on a library from before the option — CV_LIB_PATH — changes nothing: that
library has only the unkeyed route).  With either argument the record names both and every timing also carries its
quartiles; without them the shape and the record are as before.

    python tools/resolve_fused_bench.py [--reps 200] [--out profiles/resolve_fused.json] [--key-pool K] [--fused-keyed M]
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
QUARTILES = False                   # --key-pool / --fused-keyed: pct() adds p25 and p75


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
    # two parties: both sign everything; a pool: transaction t is signed by keys 2t and 2t + 1 of it, in turn
    pair = lambda t: keys if len(keys) == SIGNERS else [keys[(SIGNERS * t + j) % len(keys)] for j in range(SIGNERS)]
    wtxs = []
    for t in range(ntx):
        must = [k.public.composite for k in pair(t)]
        blob = lambda tag: bytes(rng.integers(0, 256, int(rng.integers(40, 200)), dtype=np.uint8)) + tag
        w = WireTransaction(inputs=[resolve.StateRef(prev, 0).blob], outputs=[blob(b"o0"), blob(b"o1")],
                            commands=[blob(b"c0"), blob(b"c1"), blob(b"c2")], must_sign=must)
        w._id = prev = SecureHash(host_id(w.leaves))
        wtxs.append(w)
    if len(keys) == SIGNERS:
        sigs = [k.sign_many([w._id.bytes for w in wtxs]) for k in keys]
        of = lambda t: [s[t] for s in sigs]
    else:                                                          # each key signs the transactions it is a party to
        by_tx = [[None] * SIGNERS for _ in range(ntx)]
        work = [[] for _ in keys]
        for t in range(ntx):
            for j in range(SIGNERS):
                work[(SIGNERS * t + j) % len(keys)].append((t, j))
        for k, mine in zip(keys, work):
            for (t, j), s in zip(mine, k.sign_many([wtxs[t]._id.bytes for t, _ in mine]) if mine else []):
                by_tx[t][j] = s
        of = lambda t: list(by_tx[t])
    stxs = []
    for t, w in enumerate(wtxs):
        mine = of(t)
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
    r = {"p50_ms": float(np.percentile(xs, 50)), "p99_ms": float(np.percentile(xs, 99)), "min_ms": float(xs[0]),
         "reps": int(xs.size)}
    if QUARTILES:
        r.update(p25_ms=float(np.percentile(xs, 25)), p75_ms=float(np.percentile(xs, 75)))
    return r


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
    ap.add_argument("--key-pool", type=int, default=None, help="signers drawn from this many keys (at least 2)")
    ap.add_argument("--fused-keyed", type=int, choices=(0, 1, 2), default=None, help="CV_OPT_FUSED_KEYED for the run")
    a = ap.parse_args()
    global QUARTILES
    QUARTILES = a.key_pool is not None or a.fused_keyed is not None
    if a.key_pool is not None and a.key_pool < SIGNERS:
        raise SystemExit("--key-pool: at least 2 keys")
    if not torch.cuda.is_available():
        raise SystemExit("resolve_fused_bench needs a GPU")
    engine = native.Engine(1)
    keys = [KeyPair(hashlib.sha256(b"resolve bench key %d" % k).digest(), engine) for k in range(a.key_pool or SIGNERS)]
    rec = {"tool": "tools/resolve_fused_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "timer": "perf_counter around the synchronous calls through the ctypes binding, host buffers (pageable); the "
                    "variants interleaved per repetition on the same batch, the order rotating; stages: HIP events around "
                    "the stages of one untimed call",
           "sizes": []}
    if QUARTILES:
        has = "fused_keyed" in native.OPTIONS and engine.has_option("fused_keyed")
        if a.fused_keyed is not None and (has or a.fused_keyed != 0):
            engine.set_option("fused_keyed", a.fused_keyed)
        rec.update(key_pool=a.key_pool or SIGNERS, fused_keyed=engine.get_option("fused_keyed") if has else 0,
                   library_has_fused_keyed=has, library=native.LIB_PATH)
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
