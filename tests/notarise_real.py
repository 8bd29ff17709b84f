"""The plain cases of tests/notarise_cases.py as real batches for cv_notarise_batch on the GPU, for
tests/test_gpu_fused_keyed.py: leaves, ids, signatures and requirements from which the engine computes the verdicts a
case names, in the format of tests/notarise_batches.make_batch (so notarise_batches.compose, open_set and call take
them).

A transaction's input states become its first leaves (the state's 32 bytes as the leaf, so the set's key is their
SHA-256 and two transactions share a key iff the case's share a state), followed by one leaf of its own; a transaction
without leaves has no states.  A signature (bit, status, pre) is a good signature over the true id from a pool of
eight keys, with a flipped bit for a zero verdict, under ONE key that is no point — the same for every such row, so a
bad key repeats — for CV_SIG_BAD_KEY, and carries `pre` as its sig_pre.  ck = MISSING adds a requirement nobody signed,
MALFORMED one that is no tree encoding.  What real data cannot give — a set verdict bit beside a bad-key status — is
replaced by a good signature, in the returned plain cases too.
"""
import hashlib

import numpy as np

import notarise_cases as C
from corda_amd import native


def realise(engine, corpus, txs, resident):
    """-> (batch as notarise_batches.make_batch returns it, the plain cases the batch realises)."""
    ntx = len(txs)
    bad_key = corpus["pk"][corpus["status"] == native.CV_SIG_BAD_KEY][0]
    plain = []
    for tx in txs:
        p = dict(tx)
        p["sigs"] = [(1, 0, 0) if (b, s, q) == (1, C.SIG_BAD_KEY, 0) else (b, s, q) for b, s, q in tx["sigs"]]
        if p["mstatus"]:
            p["states"] = []
        plain.append(p)
    leaves, txb, nin = [], [0], []
    for t, p in enumerate(plain):
        mine = [] if p["mstatus"] else list(p["states"]) + [b"own leaf %d" % t]
        leaves += mine
        txb.append(len(leaves))
        nin.append(len(p["states"]))
    leaf_len = np.array([len(b) for b in leaves], np.uint32)
    leaf_off = (np.cumsum(leaf_len) - leaf_len).astype(np.uint64)
    arena = np.frombuffer(b"".join(leaves) + bytes(16), np.uint8).copy()
    txb = np.array(txb, np.uint32)
    ids, _ = engine.merkle_tx_ids(arena, leaf_off, leaf_len, txb)
    nsig = [len(p["sigs"]) for p in plain]
    tsb = np.concatenate([[0], np.cumsum(nsig)]).astype(np.uint32)
    tx_of = np.repeat(np.arange(ntx), nsig)
    pool = np.array([np.frombuffer(hashlib.sha256(b"notary case key %d" % k).digest(), np.uint8) for k in range(8)])
    who = (np.arange(len(tx_of)) * 5 // 2) % 8
    pk, sig = engine.sign_batch(pool[who], ids.reshape(-1), (tx_of * 32).astype(np.uint64), np.full(len(tx_of), 32, np.uint32))
    sig_pre = np.zeros(len(tx_of), np.uint8)
    claimed, tx_pre = ids.copy(), np.zeros(ntx, np.uint8)
    stranger = hashlib.sha256(b"stranger").digest()
    kind, lkey, rb, trb, allowed = [], [], [0], [0], []
    for t, p in enumerate(plain):
        if p["claimed"] != p["recomputed"]:
            claimed[t, t % 32] ^= 0x40
        tx_pre[t] = p["tx_pre"]
        for j, (bit, status, pre) in enumerate(p["sigs"]):
            i = int(tsb[t]) + j
            if status == C.SIG_BAD_KEY:
                pk[i] = bad_key
            elif not bit:
                sig[i, 40] ^= 1
            sig_pre[i] = pre
        mine = [(native.CV_CK_LEAF, pk[int(tsb[t])].tobytes())] if p["sigs"] else []
        if p["ck"] == C.VS_MISSING:
            mine.append((native.CV_CK_LEAF, stranger))
        elif p["ck"] == C.VS_MALFORMED:
            mine.append((7, bytes(32)))
        for kd, key in mine:
            kind.append(kd), lkey.append(np.frombuffer(key, np.uint8)), rb.append(len(kind)), allowed.append(0)
        trb.append(len(rb) - 1)
    nn = len(kind)
    u32 = lambda a: np.array(a, np.uint32)
    reqs = (np.array(kind, np.uint8), np.array(lkey, np.uint8).reshape(nn, 32), np.zeros(nn, np.int32),
            np.zeros(nn + 1, np.uint32), u32([]), np.zeros(0, np.int32), u32(rb), u32(trb), pk.copy(),
            np.array(allowed, np.uint8))
    resident = dict(resident)
    resident[C.h32("unrelated")] = (C.h32("unrelated id"), 0, 0)      # the set is never loaded with nothing
    rk = list(resident)
    res = (np.array([np.frombuffer(hashlib.sha256(k).digest(), np.uint8) for k in rk], np.uint8).reshape(-1, 32),
           np.array([np.frombuffer(resident[k][0], np.uint8) for k in rk], np.uint8).reshape(-1, 32),
           u32([resident[k][1] for k in rk]), u32([resident[k][2] for k in rk]))
    batch = dict(ntx=ntx, arena=arena, leaf_off=leaf_off, leaf_len=leaf_len, tx_leaf_begin=txb, tx_input_count=u32(nin),
                 claimed=claimed, caller=u32([p["caller"] for p in plain]), tx_pre=tx_pre, pk=pk, sig=sig, tx_sig_begin=tsb,
                 sig_pre=sig_pre, reqs=reqs, leaves=leaves, resident=res)
    return batch, plain
