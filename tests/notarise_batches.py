"""Real batches for cv_notarise_batch on the GPU and their comparator, shared by tests/test_gpu_notarise.py and
tests/test_gpu_notarise_output_contract.py.

make_batch builds ntx transactions of 0 to 4 leaves with 0 to 3 inputs and 1 to 3 signatures, signed over their true
ids, with every kind of failure planted by position (t % 10), conflicts with earlier transactions of the batch and
with states loaded into the set beforehand, and a chain of conflicts at the end of the larger ones.  compose runs the
composition of the existing calls on the same inputs — cv_merkle_tx_ids_bounded -> cv_ed25519_verify_batch over the
ids -> cv_missing_signers -> the restatement of tests/notarise_cases.py for the gate -> cv_uniq_commit_batch with keys
hashlib.sha256(leaf) -> cv_ed25519_sign_keyed — and returns what cv_notarise_batch must return, array for array.
"""
import hashlib

import numpy as np

import notarise_cases as C
from corda_amd import native

KINDS = ("success", "empty", "id_mismatch", "timestamp", "tx_invalid", "bad_key", "missing", "malformed", "conflict",
         "prefilter")
NOTARY_SEED = bytes(range(32))


def _leaf(rng, tag):
    return bytes(rng.integers(0, 256, int(rng.integers(1, 90)), dtype=np.uint8)) + repr(tag).encode()


def make_batch(engine, corpus, ntx, seed=0):
    """-> dict: the arrays of Engine.notarise_batch (leaves, claimed ids, signatures, requirements), `kind` per
    transaction and `resident`: (keys, ids, index, caller) to load into the set before the call."""
    rng = np.random.default_rng(1000 * ntx + seed)
    bad_keys = corpus["pk"][corpus["status"] == native.CV_SIG_BAD_KEY]
    kinds = [KINDS[t % 10] for t in range(ntx)]
    leaves, txb, nin, first_input = [], [0], [], {}
    chain = list(range(ntx - 12, ntx)) if ntx >= 130 else []
    chain_leaf = [_leaf(rng, ("chain", j)) for j in range(13)]
    for t, k in enumerate(kinds):
        nl = 0 if k == "empty" else int(rng.integers(1, 5))
        ni = int(rng.integers(0, min(3, nl) + 1))
        if k in ("success", "conflict") and nl:
            ni = max(ni, 1)
        mine = [_leaf(rng, (t, j)) for j in range(nl)]
        if t in chain:                                     # request j of the chain holds chain states j and j + 1
            j = chain.index(t)
            kinds[t] = k = "success"
            mine = [chain_leaf[j], chain_leaf[j + 1]] + mine[:2]
            nl, ni = len(mine), 2
        elif k == "conflict" and t >= 8:
            mine[0] = first_input[t - 8]                   # an input of the accepted transaction eight before
        elif k == "success" and ni >= 2 and t % 20 == 0:
            mine[1] = mine[0]                              # a repeated input
        if k == "success" and t % 30 == 10 and nl:
            ni = nl                                        # every leaf is an input
        if ni:
            first_input[t] = mine[0]
        leaves += mine
        txb.append(len(leaves))
        nin.append(ni)
    leaf_len = np.array([len(b) for b in leaves] + [0], np.uint32)
    leaf_off = np.concatenate([[0], np.cumsum(leaf_len[:-1])]).astype(np.uint64)
    arena = np.frombuffer(b"".join(leaves) + bytes(16), np.uint8).copy()
    txb = np.array(txb, np.uint32)
    ids, _ = engine.merkle_tx_ids(arena, leaf_off[:len(leaves)], leaf_len[:len(leaves)], txb)
    # signatures over the true ids: 1 to 3 a transaction, from a pool of 8 keys
    nsig = [1 + (t + t // 3) % 3 for t in range(ntx)]
    tsb = np.concatenate([[0], np.cumsum(nsig)]).astype(np.uint32)
    tx_of = np.repeat(np.arange(ntx), nsig)
    pool = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    who = rng.integers(0, 8, len(tx_of))
    pk, sig = engine.sign_batch(pool[who], ids.reshape(-1), (tx_of * 32).astype(np.uint64), np.full(len(tx_of), 32, np.uint32))
    sig_pre = np.zeros(len(tx_of), np.uint8)
    claimed, tx_pre = ids.copy(), np.zeros(ntx, np.uint8)
    stranger = hashlib.sha256(b"stranger").digest()
    reqs, allowed = [], []                                 # per transaction: a list of requirements (lists of nodes)
    for t, k in enumerate(kinds):
        b, e = int(tsb[t]), int(tsb[t + 1])
        if k == "id_mismatch":
            claimed[t, t % 32] ^= 0x40
        elif k == "timestamp":
            tx_pre[t] = 1 + t % 200
        elif k == "tx_invalid":
            sig[e - 1, 40] ^= 1                            # the LAST signature fails: the scan walks the range
        elif k == "bad_key":
            pk[b] = bad_keys[t % len(bad_keys)]
            if e - b > 1:
                sig[b + 1, 3] ^= 1                         # a SignatureException behind it does not change the class
        elif k == "prefilter":
            sig_pre[b + (t // 10) % (e - b)] = 1 + (t // 10) % 2
        leaf = lambda key: (native.CV_CK_LEAF, bytes(key), 0, [], [])
        mine = [[leaf(pk[b])]]
        if t % 4 == 1:                                     # 1-of-2 over a signer and a stranger
            mine.append([leaf(pk[e - 1]), leaf(stranger), (native.CV_CK_NODE, bytes(32), 1, [0, 1], [1, 1])])
        ok = [0] * len(mine)
        if k == "missing":
            mine.append([leaf(stranger)])
            ok.append(0)
        elif k == "malformed":
            mine.append([(7, bytes(32), 0, [], [])])
            ok.append(0)
        elif t % 5 == 0:                                   # the notary's own key, allowed to be missing
            mine.append([leaf(hashlib.sha256(b"notary").digest())])
            ok.append(1)
        reqs.append(mine)
        allowed += ok
    kind, lkey, thr, cb, child, weight, rb, trb = [], [], [], [0], [], [], [0], [0]
    for mine in reqs:
        for req in mine:
            base = len(kind)
            for kd, key, th, ch, w in req:
                kind.append(kd), lkey.append(np.frombuffer(key, np.uint8)), thr.append(th)
                child += [base + c for c in ch]
                weight += w
                cb.append(len(child))
            rb.append(len(kind))
        trb.append(len(rb) - 1)
    u32 = lambda a: np.array(a, np.uint32)
    req_arrays = (np.array(kind, np.uint8), np.array(lkey, np.uint8), np.array(thr, np.int32), u32(cb), u32(child),
                  np.array(weight, np.int32), u32(rb), u32(trb), pk.copy(), np.array(allowed, np.uint8))
    # resident: the first input of two accepted transactions, consumed by someone else long ago
    res = [t for t in (20, 40) if t < ntx and t in first_input and kinds[t] == "success" and t not in chain]
    rkeys = np.array([np.frombuffer(hashlib.sha256(first_input[t]).digest(), np.uint8) for t in res] +
                     [np.frombuffer(hashlib.sha256(b"unrelated %d" % j).digest(), np.uint8) for j in range(3)], np.uint8)
    resident = (rkeys, rng.integers(0, 256, (len(rkeys), 32), dtype=np.uint8), np.arange(len(rkeys), dtype=np.uint32) % 3,
                np.arange(len(rkeys), dtype=np.uint32) + 100)
    return dict(ntx=ntx, kind=kinds, arena=arena, leaf_off=leaf_off[:len(leaves)], leaf_len=leaf_len[:len(leaves)],
                tx_leaf_begin=txb, tx_input_count=u32(nin), claimed=claimed, caller=u32([t % 7 for t in range(ntx)]),
                tx_pre=tx_pre, pk=pk, sig=sig, tx_sig_begin=tsb, sig_pre=sig_pre, reqs=req_arrays, leaves=leaves,
                resident=resident, expects_resident_conflict=res)


def edge_batch(engine, corpus, name):
    """One-transaction batches at which pieces of the call's one buffer are empty.  "no_inputs": the transaction has
    leaves and no input state (nstates = 0; for the simple notary).  "no_signatures": a validating call with no
    signature and no requirement at all (nsig = nreq = nnodes = nchild = 0)."""
    b = make_batch(engine, corpus, 1)
    u32 = lambda a: np.array(a, np.uint32)
    if name == "no_inputs":
        b["tx_input_count"] = u32([0])
    elif name == "no_signatures":
        none = np.zeros((0, 32), np.uint8)
        b.update(pk=none, sig=np.zeros((0, 64), np.uint8), tx_sig_begin=u32([0, 0]), sig_pre=np.zeros(0, np.uint8),
                 reqs=(np.zeros(0, np.uint8), none, np.zeros(0, np.int32), u32([0]), u32([]), np.zeros(0, np.int32),
                       u32([0]), u32([0, 0]), none, np.zeros(0, np.uint8)))
    else:
        raise KeyError(name)
    return b


def open_set(engine, batch, capacity=None):
    s = native.UniquenessSet(engine, capacity or (len(batch["resident"][0]) + int(batch["tx_input_count"].sum()) + 8))
    s.load(*batch["resident"])
    return s


def state_keys(batch):
    keys, txb = [], batch["tx_leaf_begin"]
    for t in range(batch["ntx"]):
        for j in range(int(batch["tx_input_count"][t])):
            keys.append(np.frombuffer(hashlib.sha256(batch["leaves"][int(txb[t]) + j]).digest(), np.uint8))
    return np.array(keys, np.uint8).reshape(-1, 32)


def call(engine, uniq, signer, b, validating=True, out=None):
    return engine.notarise_batch(uniq, signer, b["arena"], b["leaf_off"], b["leaf_len"], b["tx_leaf_begin"],
                                 b["tx_input_count"], b["claimed"], b["caller"], b["tx_pre"],
                                 sigs=(b["pk"], b["sig"], b["tx_sig_begin"], b["sig_pre"]) if validating else None,
                                 reqs=b["reqs"] if validating else None, out=out)


def compose(engine, signer, b, validating=True):
    """The five existing calls and the restatement's gate on a fresh set loaded like the fused call's -> (the expected
    outputs by name, the set afterwards)."""
    ntx, tsb = b["ntx"], b["tx_sig_begin"]
    ids, mst = engine.merkle_tx_ids(b["arena"], b["leaf_off"], b["leaf_len"], b["tx_leaf_begin"])
    nsig = int(tsb[-1])
    tx_of = np.repeat(np.arange(ntx), np.diff(tsb))
    req_missing = np.zeros(0, np.uint8)
    bits, sst, ck = np.ones(nsig, bool), np.zeros(nsig, np.uint8), np.zeros(ntx, np.uint8)
    if validating:
        bm = np.zeros(0, np.uint64)
        if nsig:
            bm, sst = engine.verify_batch(b["pk"], b["sig"], ids.reshape(-1), (tx_of * 32).astype(np.uint64),
                                          np.full(nsig, 32, np.uint32))
            bits = native.bitmap_to_bools(bm, nsig)
        r = b["reqs"]
        req_missing, ck = engine.missing_signers(*r[:9], tsb, req_allowed=r[9], bitmap=bm)
    txs = [dict(mstatus=int(mst[t]), recomputed=ids[t].tobytes(), claimed=b["claimed"][t].tobytes(), tx_pre=int(b["tx_pre"][t]),
                sigs=[(int(bits[i]), int(sst[i]), int(b["sig_pre"][i])) for i in range(int(tsb[t]), int(tsb[t + 1]))],
                ck=int(ck[t])) for t in range(ntx)]
    pre, enable, first_bad = C.gate(txs, 1 if validating else 0)
    uniq = open_set(engine, b)
    sbeg = np.concatenate([[0], np.cumsum(b["tx_input_count"])]).astype(np.uint32)
    ust, sc, cid, cix, cc = uniq.commit_batch(state_keys(b), sbeg, ids, b["caller"], enable)
    outcome = np.where((enable == 1) & (ust == native.CV_UNIQ_CONFLICT), C.CONFLICT, pre).astype(np.uint8)
    acc = np.flatnonzero(outcome == C.SUCCESS)
    nsigs = np.zeros((ntx, 64), np.uint8)
    if len(acc):
        nsigs[acc] = signer.sign(ids.reshape(-1), (acc * 32).astype(np.uint64), np.full(len(acc), 32, np.uint32))
    return dict(outcome=outcome, ids=ids, notary_sig=nsigs, first_bad=first_bad, req_missing=req_missing, state_conflict=sc,
                consumed_id=cid, consumed_index=cix, consumed_caller=cc), uniq


def same_sets(a, b, keys):
    """Both sets hold the same records for every key, and the same number of them."""
    ra, rb = a.lookup(keys), b.lookup(keys)
    return all(np.array_equal(x, y) for x, y in zip(ra, rb)) and a.stats()["resident"] == b.stats()["resident"]
