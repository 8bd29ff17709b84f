#!/usr/bin/env python3
"""What notarising a batch costs end to end from host buffers: the five existing C-ABI calls with numpy glue between
them (A: what a binding had before cv_notarise_batch) against the one fused call (B), DESIGN.md §5.11.

Shape C4: ntx transactions x 8 signers (256, 4,096 and 65,536 signatures), 6 leaves a transaction (workload.LEAF_SHAPE)
of which the first 2 are inputs, one Leaf requirement per signer, every 16th signature record replaced by one of the
golden corpus's rejected records (workload.adversarial_records), so one transaction in two fails its signature check.
A and B run interleaved in one process, one repetition after the other on the same batch, each on its own uniqueness
set; their outcomes and notary signatures are compared in every repetition.  Batches are generated beforehand (K of
them, each with leaves — so inputs — of its own); every K repetitions both sets are closed, reopened with the capacity
reserved and warmed with one untimed call on a spare batch, so the inputs of every timed call are new to its set and no
timed call grows a table or a workspace.  Timed with the host clock around the synchronous calls, inputs prepared and
outputs allocated by the binding inside the timed span for both.  A's C calls are also summed on their own
(`a_calls`): the difference to `a` is its numpy / hashlib glue (the state keys are hashlib.sha256 of the input leaves).
Reports p50 and p99 and the verify-only p50 (cv_ed25519_verify_batch over the same signatures) for scale.
Writes one JSON record (default profiles/notary_fused.json).  Needs a GPU: no fallback.

--key-pool K signs every record with one of K keys instead of a key of its own (the corpus's rejected records keep
theirs), the shape the keyed verify route is for; --fused-keyed {0,1,2} sets CV_OPT_FUSED_KEYED for the run (0 on a
library from before the option — CV_LIB_PATH — changes nothing: that library has only the unkeyed route).  With either
argument the record names both and every timing also carries its quartiles; without them the shape
and the record are as before.

    python tools/notary_fused_bench.py [--reps 200] [--out profiles/notary_fused.json] [--key-pool K] [--fused-keyed M]
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

SIGNERS, LEAVES, INPUTS = 8, len(workload.LEAF_SHAPE), 2
SIZES = (256, 4096, 65536)
K = 25
NO_SIG = native.NS_NO_SIG


QUARTILES = False                   # --key-pool / --fused-keyed: pct() adds p25 and p75


def make(engine, ntx, seed, adversarial, key_pool=0):
    tb = workload.make_tx_batch(engine, 0, ntx, signers=SIGNERS, seed=seed)
    h = lambda t, dt: t.cpu().numpy().astype(dt)
    n = ntx * SIGNERS
    pk, sig = h(tb.sigs.pk, np.uint8), h(tb.sigs.sig, np.uint8)
    if key_pool:                    # the same pool for every batch of the run, so its keys stay resident
        pool = np.random.default_rng(key_pool).integers(0, 256, (key_pool, 32), dtype=np.uint8)
        who = np.random.default_rng(seed).integers(0, key_pool, n)
        pk, sig = engine.sign_batch(pool[who], h(tb.ids, np.uint8).reshape(-1), (np.arange(n, dtype=np.uint64) // SIGNERS) * 32,
                                    np.full(n, 32, np.uint32))
    apk, asig, _ = adversarial
    for j, i in enumerate(range(seed % 16, n, 16)):
        pk[i], sig[i] = apk[j % len(apk)], asig[j % len(apk)]
    one = np.arange(n + 1, dtype=np.uint32)
    b = dict(ntx=ntx, arena=h(tb.leaf_arena, np.uint8), leaf_off=h(tb.leaf_off, np.uint64), leaf_len=h(tb.leaf_len, np.uint32),
             txb=h(tb.tx_begin, np.uint32), nin=np.full(ntx, INPUTS, np.uint32), claimed=h(tb.ids, np.uint8),
             caller=(np.arange(ntx) % 16).astype(np.uint32), pk=pk, sig=sig,
             tsb=np.arange(0, n + 1, SIGNERS, dtype=np.uint32), msg_off=(np.arange(n, dtype=np.uint64) // SIGNERS) * 32,
             msg_len=np.full(n, 32, np.uint32), sbeg=np.arange(0, INPUTS * ntx + 1, INPUTS, dtype=np.uint32))
    # one Leaf requirement per signer: node k = requirement k = signature k's key
    b["reqs"] = (np.zeros(n, np.uint8), pk, np.zeros(n, np.int32), np.zeros(n + 1, np.uint32), np.zeros(0, np.uint32),
                 np.zeros(0, np.int32), one, b["tsb"], pk, None)
    return b


def run_a(engine, uniq, signer, b):
    """The five calls and the decisions between them -> (outcome, notary_sig, seconds inside the C calls)."""
    ntx, tsb = b["ntx"], b["tsb"]
    calls = 0.0
    t = time.perf_counter()
    ids, mst = engine.merkle_tx_ids(b["arena"], b["leaf_off"], b["leaf_len"], b["txb"])
    calls += time.perf_counter() - t
    t = time.perf_counter()
    bm, sst = engine.verify_batch(b["pk"], b["sig"], ids.reshape(-1), b["msg_off"], b["msg_len"])
    calls += time.perf_counter() - t
    t = time.perf_counter()
    r = b["reqs"]
    _, ck = engine.missing_signers(*r[:9], tsb, req_allowed=None, bitmap=bm)
    calls += time.perf_counter() - t
    # the gate (NotaryFlow.kt:96-113, ValidatingNotaryFlow.kt:24-45), vectorised
    bits = native.bitmap_to_bools(bm, int(tsb[-1]))
    idx = np.where(bits, NO_SIG, np.arange(bits.size, dtype=np.uint32))
    first = np.minimum.reduceat(idx, tsb[:-1])
    bad = first != NO_SIG
    cls = np.where(sst[np.where(bad, first, 0)] == native.CV_SIG_BAD_KEY, native.CV_NS_BAD_KEY, native.CV_NS_TX_INVALID)
    pre = np.where(ck == native.CV_VS_MALFORMED, native.CV_NS_MALFORMED,
                   np.where(ck == native.CV_VS_MISSING, native.CV_NS_SIGNATURES_MISSING, native.CV_NS_SUCCESS))
    pre = np.where(bad, cls, pre)
    pre = np.where((ids != b["claimed"]).any(1), native.CV_NS_ID_MISMATCH, pre)
    pre = np.where(mst != 0, native.CV_NS_EMPTY, pre).astype(np.uint8)
    enable = (pre == 0).astype(np.uint8)
    arena, off, ln, txb = b["arena"], b["leaf_off"], b["leaf_len"], b["txb"]
    keys = np.frombuffer(b"".join(hashlib.sha256(arena[int(off[l]):int(off[l]) + int(ln[l])]).digest()
                                  for t0 in txb[:-1] for l in range(int(t0), int(t0) + INPUTS)), np.uint8)
    t = time.perf_counter()
    ust = uniq.commit_batch(keys, b["sbeg"], ids, b["caller"], enable)[0]
    calls += time.perf_counter() - t
    outcome = np.where((enable == 1) & (ust == native.CV_UNIQ_CONFLICT), native.CV_NS_CONFLICT, pre).astype(np.uint8)
    acc = np.flatnonzero(outcome == 0)
    nsig = np.zeros((ntx, 64), np.uint8)
    t = time.perf_counter()
    if acc.size:
        nsig[acc] = signer.sign(ids.reshape(-1), (acc * 32).astype(np.uint64), np.full(acc.size, 32, np.uint32))
    calls += time.perf_counter() - t
    return outcome, nsig, calls


def run_b(engine, uniq, signer, b):
    out = engine.notarise_batch(uniq, signer, b["arena"], b["leaf_off"], b["leaf_len"], b["txb"], b["nin"], b["claimed"],
                                b["caller"], None, sigs=(b["pk"], b["sig"], b["tsb"], None), reqs=b["reqs"])
    return out["outcome"], out["notary_sig"]


def pct(xs):
    xs = np.sort(np.array(xs)) * 1e3
    r = {"p50_ms": float(np.percentile(xs, 50)), "p99_ms": float(np.percentile(xs, 99)), "min_ms": float(xs[0]),
         "reps": int(xs.size)}
    if QUARTILES:
        r.update(p25_ms=float(np.percentile(xs, 25)), p75_ms=float(np.percentile(xs, 75)))
    return r


def one_size(engine, signer, nsig, reps, adversarial, key_pool=0):
    ntx = nsig // SIGNERS
    batches = [make(engine, ntx, 1000 * nsig + j, adversarial, key_pool) for j in range(K + 1)]
    ta, tb, tac, tv, sets = [], [], [], [], []
    accepted = None
    for rep in range(reps):
        j = rep % K
        if j == 0:
            for s in sets:
                s.close()
            sets = [native.UniquenessSet(engine, (K + 2) * ntx * INPUTS) for _ in range(2)]
            run_a(engine, sets[0], signer, batches[K])
            run_b(engine, sets[1], signer, batches[K])
        b = batches[j]
        order = (0, 1) if rep % 2 == 0 else (1, 0)             # alternate who goes first
        res = {}
        for which in order:
            t = time.perf_counter()
            res[which] = run_a(engine, sets[0], signer, b) if which == 0 else run_b(engine, sets[1], signer, b)
            (ta if which == 0 else tb).append(time.perf_counter() - t)
        tac.append(res[0][2])
        if not (np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])):
            raise SystemExit(f"nsig={nsig} rep {rep}: the fused call and the five calls disagree")
        accepted = int((res[1][0] == 0).sum())
        t = time.perf_counter()
        engine.verify_batch(b["pk"], b["sig"], b["claimed"].reshape(-1), b["msg_off"], b["msg_len"])
        tv.append(time.perf_counter() - t)
    for s in sets:
        s.close()
    rec = {"signatures": nsig, "ntx": ntx, "signers": SIGNERS, "leaves": LEAVES, "inputs": INPUTS, "batches": K,
           "accepted_last_batch": accepted, "a_five_calls": pct(ta), "a_calls_only": pct(tac), "b_fused": pct(tb),
           "verify_only": pct(tv)}
    rec["a_over_b_p50"] = rec["a_five_calls"]["p50_ms"] / rec["b_fused"]["p50_ms"]
    rec["a_calls_only_over_b_p50"] = rec["a_calls_only"]["p50_ms"] / rec["b_fused"]["p50_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "notary_fused.json"))
    ap.add_argument("--key-pool", type=int, default=None, help="signers drawn from this many keys")
    ap.add_argument("--fused-keyed", type=int, choices=(0, 1, 2), default=None, help="CV_OPT_FUSED_KEYED for the run")
    a = ap.parse_args()
    global QUARTILES
    QUARTILES = a.key_pool is not None or a.fused_keyed is not None
    if a.reps < 200:
        raise SystemExit("at least 200 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("notary_fused_bench needs a GPU")
    engine = native.Engine(1)
    signer = native.Signer(engine, bytes(range(32)))
    adversarial = workload.adversarial_records(os.path.join(REPO, "tests", "golden", "ed25519_corpus.npz"))
    rec = {"tool": "tools/notary_fused_bench.py", "device": torch.cuda.get_device_name(0),
           "timer": "perf_counter around the synchronous calls through the ctypes binding, host buffers (pageable); A and B "
                    "interleaved per repetition on the same batch, the order alternating",
           "sizes": []}
    if QUARTILES:
        has = "fused_keyed" in native.OPTIONS and engine.has_option("fused_keyed")
        if a.fused_keyed is not None and (has or a.fused_keyed != 0):
            engine.set_option("fused_keyed", a.fused_keyed)
        rec.update(key_pool=a.key_pool or 0, fused_keyed=engine.get_option("fused_keyed") if has else 0,
                   library_has_fused_keyed=has, library=native.LIB_PATH)
    ok = True
    for n in a.sizes:
        r = one_size(engine, signer, n, a.reps, adversarial, a.key_pool or 0)
        rec["sizes"].append(r)
        ok &= r["b_fused"]["p50_ms"] <= r["a_five_calls"]["p50_ms"]
        print(f"sigs={n:6d}  A five calls p50 {r['a_five_calls']['p50_ms']:.3f} p99 {r['a_five_calls']['p99_ms']:.3f} ms "
              f"(C calls alone p50 {r['a_calls_only']['p50_ms']:.3f})  B fused p50 {r['b_fused']['p50_ms']:.3f} p99 "
              f"{r['b_fused']['p99_ms']:.3f} ms  verify only p50 {r['verify_only']['p50_ms']:.3f} ms  A/B {r['a_over_b_p50']:.2f}",
              flush=True)
    rec["b_p50_not_above_a_p50_everywhere"] = bool(ok)
    signer.close()
    engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    if not ok:
        raise SystemExit("the fused call's p50 is above the five calls' at some size")


if __name__ == "__main__":
    main()
