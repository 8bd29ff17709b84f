#!/usr/bin/env python3
"""Measures cv_missing_signers on one MI355X (the record is profiles/ck_probe.json).

    python tools/ck_probe.py [--out profiles/ck_probe.json] [--ntx-c3 1000000]

(a) the notary shape from host buffers: 4,096 transactions, three mustSign entries each (one a 1-of-2 Node, one the
    notary's key, which is allowed to be missing), two signers — the p50 of the synchronous host call (host clock
    around it: the call ends in a stream synchronise), of the mirror's flattening, and, beside them in the same run,
    of the per-transaction `_finish_verify` loop the call replaces.
(b) the C3 shape, device-resident: 1M transactions x 8 signers with 2-8 Leaf requirements each — the device form's
    time (HIP events on the stream) and its share of the device-resident C3 step on the same box (Merkle ids + 8M
    verifies, what cv_verify_transactions runs on the device) and of the synchronous cv_verify_transactions over the
    same transactions from pinned host buffers; and the notary-shaped 4,096-transaction batch in the device form
    with wide_min at its default and at both extremes.
Warm-up first, medians reported, every timed call's results checked.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from corda_amd import native, workload  # noqa: E402
from corda_amd.crypto import CompositeKey, DigitalSignature, EdDSAPublicKey  # noqa: E402
from corda_amd.transactions import (SecureHash, SignedTransaction, WireTransaction, flatten_must_sign,  # noqa: E402
                                    missing_signatures_batch)

FLAT = ("kind", "leaf_key", "threshold", "child_begin", "child", "weight", "req_begin", "tx_req_begin", "sig_key",
        "tx_sig_begin")


def p50(xs):
    return float(np.median(np.array(xs)))


def notary_shape(ntx, rng):
    notary = EdDSAPublicKey(rng.integers(0, 256, 32, dtype=np.uint8).tobytes()).composite
    stxs = []
    for t in range(ntx):
        a, b, c = (EdDSAPublicKey(rng.integers(0, 256, 32, dtype=np.uint8).tobytes()) for _ in range(3))
        must = [a.composite, notary, CompositeKey.Node(1, [b.composite, c.composite], [1, 1])]
        wtx = WireTransaction(inputs=[b"in"], must_sign=must, notary_key=notary)
        wtx._id = SecureHash(rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
        stxs.append(SignedTransaction(wtx, [DigitalSignature.WithKey(a, bytes(64)), DigitalSignature.WithKey(b, bytes(64))],
                                      wtx._id))
    return stxs, notary


def timed_device(fn, warm=5, reps=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return p50(ms), float(min(ms)), float(max(ms))


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to("cuda:0")


def device_call(eng, d, counts, wide_min, rm, st, ws, stream):
    ntx, nreq, nnodes, nchild, nsig = counts
    return lambda: eng.missing_signers_device(0, ntx, nreq, nnodes, nchild, nsig, *[d[k].data_ptr() for k in FLAT],
                                              d["req_allowed"].data_ptr() if "req_allowed" in d else 0, 0, wide_min,
                                              rm.data_ptr(), st.data_ptr(), ws.data_ptr(), stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ck_probe.json")
    ap.add_argument("--ntx-notary", type=int, default=4096)
    ap.add_argument("--ntx-c3", type=int, default=1_000_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ck_probe needs a GPU")
    eng = native.Engine(1)
    rng = np.random.default_rng(20261020)
    rec = {"device": torch.cuda.get_device_name(0), "version": native.load().cv_version().decode()}

    # ---- (a) notary shape, host buffers
    stxs, notary = notary_shape(args.ntx_notary, rng)
    t_flat = []
    for _ in range(7):
        t0 = time.perf_counter()
        f = flatten_must_sign(stxs, (notary,))
        t_flat.append((time.perf_counter() - t0) * 1e3)
    call = lambda: eng.missing_signers(**f)  # noqa: E731
    for _ in range(20):
        rm, st = call()
    assert (st == native.CV_VS_OK).all() and int((rm == 1).sum()) == args.ntx_notary
    t_call = []
    for _ in range(200):
        t0 = time.perf_counter()
        call()
        t_call.append((time.perf_counter() - t0) * 1e3)
    t_batch, t_loop = [], []
    for _ in range(7):
        t0 = time.perf_counter()
        out = missing_signatures_batch(stxs, (notary,), eng)
        t_batch.append((time.perf_counter() - t0) * 1e3)
        assert all(e is None for e in out)
        t0 = time.perf_counter()
        for s in stxs:
            s._finish_verify((notary,))
        t_loop.append((time.perf_counter() - t0) * 1e3)
    counts = (len(stxs), f["req_begin"].size - 1, f["kind"].size, f["child"].size, f["sig_key"].shape[0])
    rec["notary_host"] = {"ntx": counts[0], "nreq": counts[1], "nnodes": counts[2], "nsig": counts[4],
                          "cv_missing_signers_p50_ms": p50(t_call), "cv_missing_signers_min_ms": float(min(t_call)),
                          "flatten_must_sign_p50_ms": p50(t_flat), "missing_signatures_batch_p50_ms": p50(t_batch),
                          "finish_verify_loop_p50_ms": p50(t_loop)}

    # ---- (b) the same batch, device form, wide_min at the default and both extremes
    # one stream of this program's for torch's work, the engine's and the timing events (the null stream's handle, 0,
    # would mean "the context's own stream" to the engine)
    ts = torch.cuda.Stream("cuda:0")
    torch.cuda.set_stream(ts)
    stream = ts.cuda_stream
    d = {k: up(f[k]) for k in FLAT + ("req_allowed",)}
    rm_d = torch.empty(counts[1], dtype=torch.uint8, device="cuda:0")
    st_d = torch.empty(counts[0], dtype=torch.uint8, device="cuda:0")
    ws = torch.empty(native.missing_signers_workspace(counts[0], counts[2]), dtype=torch.uint8, device="cuda:0")
    rec["notary_device"] = {}
    for name, wm in (("default", 0), ("always_wide", 1), ("never_wide", 0xFFFFFFFF)):
        ms = timed_device(device_call(eng, d, counts, wm, rm_d, st_d, ws, stream))
        assert int(st_d.sum()) == 0 and np.array_equal(rm_d.cpu().numpy(), rm)
        rec["notary_device"][name] = {"p50_ms": ms[0], "min_ms": ms[1], "max_ms": ms[2]}

    # ---- (b) C3 shape: 1M transactions x 8 signers, 2-8 Leaf requirements each
    ntx, signers = args.ntx_c3, 8
    tb = workload.make_tx_batch(eng, 0, ntx, signers, stream=stream)
    n = tb.sigs.n
    g = torch.Generator(device="cuda:0")
    g.manual_seed(7)
    cnt = torch.randint(2, 9, (ntx,), device="cuda:0", generator=g)
    trb = torch.zeros(ntx + 1, dtype=torch.int64, device="cuda:0")
    trb[1:] = torch.cumsum(cnt, 0)
    nreq = int(trb[-1])
    tx_of = torch.repeat_interleave(torch.arange(ntx, device="cuda:0"), cnt)
    j = torch.arange(nreq, device="cuda:0") - trb[tx_of]
    c3 = {"kind": torch.zeros(nreq, dtype=torch.uint8, device="cuda:0"),
          "leaf_key": tb.sigs.pk.view(ntx, signers, 32)[tx_of, j].contiguous(),
          "threshold": torch.zeros(nreq, dtype=torch.int32, device="cuda:0"),
          "child_begin": torch.zeros(nreq + 1, dtype=torch.int32, device="cuda:0"),
          "child": torch.zeros(4, dtype=torch.int32, device="cuda:0"), "weight": torch.zeros(4, dtype=torch.int32, device="cuda:0"),
          "req_begin": torch.arange(nreq + 1, dtype=torch.int32, device="cuda:0"), "tx_req_begin": trb.to(torch.int32),
          "sig_key": tb.sigs.pk, "tx_sig_begin": tb.sig_tx_begin.to(torch.int32)}
    c3_counts = (ntx, nreq, nreq, 0, n)
    rm3 = torch.empty(nreq, dtype=torch.uint8, device="cuda:0")
    st3 = torch.empty(ntx, dtype=torch.uint8, device="cuda:0")
    ws3 = torch.empty(native.missing_signers_workspace(ntx, nreq), dtype=torch.uint8, device="cuda:0")
    ck = timed_device(device_call(eng, c3, c3_counts, 0, rm3, st3, ws3, stream), warm=3, reps=15)
    assert int(st3.sum()) == 0 and int(rm3.sum()) == 0
    nleaves = int(tb.leaf_len.numel())
    ids = torch.empty_like(tb.ids)
    mws = torch.empty(nleaves * 32, dtype=torch.uint8, device="cuda:0")
    bitmap = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda:0")

    def c3_step():
        eng.merkle_device(0, ntx, nleaves, tb.leaf_arena.data_ptr(), tb.leaf_off.data_ptr(), tb.leaf_len.data_ptr(),
                          tb.tx_begin.data_ptr(), mws.data_ptr(), ids.data_ptr(), 0, stream)
        eng.verify_device(0, n, tb.sigs.pk.data_ptr(), tb.sigs.sig.data_ptr(), tb.sigs.arena.data_ptr(),
                          tb.sigs.off.data_ptr(), tb.sigs.len.data_ptr(), bitmap.data_ptr(), 0, stream)
    step = timed_device(c3_step, warm=2, reps=7)
    # cv_verify_transactions itself, synchronous, the same transactions from pinned host buffers
    pin = lambda t: eng.host_copy(t.cpu().numpy())  # noqa: E731
    vt_args = (pin(tb.leaf_arena), eng.host_copy(tb.leaf_off.cpu().numpy().astype(np.uint64)),
               eng.host_copy(tb.leaf_len.cpu().numpy().astype(np.uint32)),
               eng.host_copy(tb.tx_begin.cpu().numpy().astype(np.uint32)), pin(tb.sigs.pk), pin(tb.sigs.sig),
               eng.host_copy(np.arange(0, n + 1, signers, dtype=np.uint32)))
    ids_host = eng.host_empty((ntx, 32))
    t_vt = []
    for k in range(3 + 7):
        t0 = time.perf_counter()
        ok, _, _, _ = eng.verify_transactions(*vt_args, ids=ids_host, want_status=False)
        if k >= 3:
            t_vt.append((time.perf_counter() - t0) * 1e3)
        assert ok.all(), "cv_verify_transactions rejected an honest transaction"
    bytes_read = 32 * nreq + 32 * n + 4 * (2 * nreq + 2 * ntx) + nreq       # keys both sides, ranges, kinds
    rec["c3_device"] = {"ntx": ntx, "nreq": nreq, "nsig": n, "cv_missing_signers_device_p50_ms": ck[0],
                        "min_ms": ck[1], "max_ms": ck[2], "c3_step_merkle_plus_verify_p50_ms": step[0],
                        "share_of_c3_step": ck[0] / step[0],
                        "cv_verify_transactions_pinned_host_p50_ms": p50(t_vt),
                        "share_of_cv_verify_transactions": ck[0] / p50(t_vt), "input_bytes": bytes_read,
                        "input_gb_per_s": bytes_read / (ck[0] * 1e-3) / 1e9}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))
    eng.close()


if __name__ == "__main__":
    main()
