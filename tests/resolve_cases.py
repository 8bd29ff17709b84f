"""Cases and the reference restatement for cv_resolve_batch, shared by tests/test_resolve_cpu.py (the lane functions
and the host order / walk of corda_amd/csrc/cv_resolve.h on the CPU), tests/test_gpu_resolve.py and
tests/test_gpu_resolve_output_contract.py (the entry point on the GPU).  Pure Python but for `real`, which signs with
the engine.

resolve_ref is the body of ResolveTransactionsFlow.call (ResolveTransactionsFlow.kt:96-111) with topologicalSort
(:37-67), the duplicate check (:170) and loadState (ServiceHub.kt:46-49) over plain data, written as the reference's
control flow: dicts keyed by the id bytes, visit() recursive, exceptions thrown where the reference throws them.  A
transaction is a dict of tests/notarise_cases.py (mstatus, claimed, recomputed, sigs, ck: what verifySignatures sees)
with  inputs [(txhash bytes, index)]  and  nout  (the number of its outputs).

A case is SYMBOLIC, a list of specs  dict(inputs=[(ref, index)], nout, faults, same_as)  — ref an index of the batch
or a string naming a transaction outside it, same_as the index of a transaction whose leaves (so whose id) this one
repeats.  concrete() turns it into plain transactions with made-up ids and verdicts (the CPU harness), real() into
leaves and signatures the engine computes the same verdicts from.
"""
import hashlib
import sys

import numpy as np

import notarise_cases as NC

OK, EMPTY, ID_MISMATCH, TX_INVALID, BAD_KEY, SIGNATURES_MISSING, MALFORMED, BAD_INPUT, UNRESOLVED = 0, 1, 2, 4, 5, 6, 7, 9, 10
NONE = 0xFFFFFFFF
G_OK, G_BAD_ID, G_DUPLICATE_ID = 0, 1, 2
G_WORDS = ("status", "which", "n_pass", "stop_class", "stop_tx", "stop_input", "external", "maxprobe", "wraps")
G_COMPARED = 7                    # maxprobe and wraps are diagnostics of the table: they depend on the seed
SIZES = (1, 2, 64, 65, 1025, 5000)
WRAP_SEED = 0xA3                  # chain(65) as real() builds it: a probe passes the table's last slot (test_resolve_cpu)


# ---------------------------------------------------------------- the reference, restated
class Stop(Exception):
    """What ends the loop of :105-111: the exception's class as the call's code, the transaction, the input."""


    def __init__(self, cls, tx, inp):
        super().__init__(cls)
        self.cls, self.tx, self.inp = cls, tx, inp


def _topological_sort(txs):
    """:37-67 literally; transactions are their indices, SignedTransaction.id is txs[t]["claimed"]."""
    forward = {}
    for t, tx in enumerate(txs):
        for h, _ in tx["inputs"]:
            forward.setdefault(h, {})[t] = None           # LinkedHashSet: insertion order, no repeats
    visited, result = set(), []

    def visit(t):
        if txs[t]["claimed"] not in visited:
            visited.add(txs[t]["claimed"])
            for d in forward.get(txs[t]["claimed"], ()):
                visit(d)
            result.append(t)

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4 * len(txs) + 1000))
    try:
        for t in range(len(txs)):
            visit(t)
    finally:
        sys.setrecursionlimit(limit)
    result.reverse()
    assert len(result) == len(txs)
    return result


def resolve_ref(txs):
    """-> the outputs of cv_resolve_batch by name (graph without its two diagnostics)."""
    n = len(txs)
    pre, _, first_bad = NC.gate(txs, 1)                    # the `tx` getter and verifySignatures(), per transaction
    first = {}
    for t, tx in enumerate(txs):
        first.setdefault(tx["claimed"], t)
    dep, status, tib = [], [], [0]
    for tx in txs:
        for h, idx in tx["inputs"]:
            d = first.get(h, NONE)
            dep.append(d)
            status.append(0 if d == NONE else 1 if idx < txs[d]["nout"] else 2)
        tib.append(len(dep))
    outcome, bad_input = pre.copy(), np.full(n, NONE, np.uint32)
    for t in range(n):
        bad = [i for i in range(tib[t], tib[t + 1]) if status[i] == 2]
        if pre[t] == OK and bad:
            outcome[t], bad_input[t] = BAD_INPUT, bad[0]
    g = dict(status=G_OK, which=NONE, n_pass=0, stop_class=NONE, stop_tx=NONE, stop_input=NONE, external=status.count(0))
    order = [0] * n
    bad_id = [t for t in range(n) if pre[t] in (EMPTY, ID_MISMATCH)]
    count = {}
    for tx in txs:
        count[tx["claimed"]] = count.get(tx["claimed"], 0) + 1
    dup = [t for t in range(n) if count[txs[t]["claimed"]] > 1]
    if bad_id:                                            # :167 / :41: stx.tx of every download, before anything else
        g.update(status=G_BAD_ID, which=bad_id[0])
    elif dup:                                             # :170
        g.update(status=G_DUPLICATE_ID, which=dup[0])
    else:
        order = _topological_sort(txs)
        recorded = {}                                     # storageService.validatedTransactions, the batch's part
        g["n_pass"] = n
        try:
            for p, t in enumerate(order):                 # :105-111
                if pre[t] != OK:
                    raise Stop(int(pre[t]), t, NONE)      # stx.toLedgerTransaction -> verifySignatures()
                for i, (h, idx) in enumerate(txs[t]["inputs"]):        # loadState, input by input
                    if h not in first:
                        continue                          # not downloaded: the node stores it already
                    if h not in recorded:
                        raise Stop(UNRESOLVED, t, tib[t] + i)
                    if idx >= txs[recorded[h]]["nout"]:
                        raise Stop(BAD_INPUT, t, tib[t] + i)
                recorded[txs[t]["claimed"]] = t
        except Stop as s:
            g.update(n_pass=order.index(s.tx), stop_class=s.cls, stop_tx=s.tx, stop_input=s.inp)
    return dict(outcome=outcome, first_bad=first_bad, bad_input=bad_input, input_dep=np.array(dep, np.uint32),
                input_status=np.array(status, np.uint8), order=np.array(order, np.uint32),
                graph=np.array([g[k] for k in G_WORDS[:G_COMPARED]], np.uint32))


# ---------------------------------------------------------------- symbolic cases
def spec(inputs=(), nout=1, faults=(), same_as=None):
    return dict(inputs=list(inputs), nout=nout, faults=set(faults), same_as=same_as)


def _fill(core, n):
    """core, then independent transactions with one outside input each, up to n; None when core does not fit."""
    if len(core) > n:
        return None
    return core + [spec([("fill%d" % t, 0)]) for t in range(len(core), n)]


def chain(n, faults_at=None, faults=()):
    """Download order: the newest first, each spending output 0 of the next (the breadth-first download's order)."""
    c = [spec([(t + 1, 0)] if t + 1 < n else [("genesis", 0)]) for t in range(n)]
    if faults_at is not None:
        c[faults_at]["faults"] = set(faults)
    return c


def chain_reversed(n):
    return [spec([(t - 1, 0)] if t else [("genesis", 0)]) for t in range(n)]


def _mid(fault):
    return lambda n: chain(n, n // 2, (fault,)) if n >= 3 else None


def _index_edges(n):
    return _fill([spec([(1, 2)]), spec([("a", 0)], nout=3), spec([(1, 3)]), spec([("b", 1), (1, 0xFFFFFFFF)]),
                  spec([("c", 0)], nout=0), spec([(4, 0)])], n)


def _dup(n):
    # the id at indices (1, 2, 3); transaction 0 spends it; another pair further on
    return _fill([spec([(2, 0)]), spec([("d", 0)]), spec([("d", 0)], same_as=1), spec([("d", 0)], same_as=1),
                  spec([("e", 0)]), spec([("e", 0)], same_as=4)], n)


# every pair of stop conditions in one transaction (index 0; transaction 1 is its dependency with one output)
_COND = {"id_mismatch": (("id_mismatch",), []), "bad_sig": (("bad_sig",), []), "missing": (("missing",), []),
         "bad_input": ((), [(1, 1)]), "unresolved": ((), [(0, 0)])}


def _pair(a, b):
    def build(n):
        fa, ia = _COND[a]
        fb, ib = _COND[b]
        return _fill([spec(ia + ib + [(1, 0)], faults=fa + fb), spec([("p", 0)])], n)
    return build


CASES = {
    "chain": chain,
    "chain_reversed": chain_reversed,
    "diamond": lambda n: _fill([spec([(1, 0), (2, 0)]), spec([(3, 0)]), spec([(3, 1)]), spec([("g", 0)], nout=2)], n),
    "two_inputs_one_dependency": lambda n: _fill([spec([(1, 0), (1, 1), (1, 0)]), spec([("g", 0)], nout=2)], n),
    "fan_in": lambda n: _fill([spec([(t, 0) for t in range(1, 301)])] + [spec([("g%d" % t, 0)]) for t in range(300)], n),
    "fan_out": lambda n: _fill([spec([("g", 0)], nout=2000)] + [spec([(0, t)]) for t in range(2000)], n),
    "external_only": lambda n: _fill([], n),
    "no_inputs": lambda n: [spec() for _ in range(n)],
    "index_edges": _index_edges,
    "self_reference": lambda n: _fill([spec([(0, 0)])], n),
    "two_cycle": lambda n: _fill([spec([(1, 0)]), spec([(0, 0)])], n),
    "cycle_off_chain": lambda n: _fill([spec([(1, 0)]), spec([(2, 0)]), spec([(3, 0)]), spec([(2, 0), ("g", 0)])], n),
    "duplicate_id": _dup,
    "bad_signature_mid_chain": _mid("bad_sig"),
    "bad_key_mid_chain": _mid("bad_key"),
    "missing_signer_mid_chain": _mid("missing"),
    "id_mismatch_mid_chain": _mid("id_mismatch"),
    "empty_mid_chain": _mid("empty"),
    "no_signatures": lambda n: _fill([spec([(1, 0)], faults=("nosig",)), spec([("g", 0)])], n),
    "malformed_requirement": lambda n: _fill([spec([(1, 0)], faults=("malformed",)), spec([("g", 0)])], n),
    "unresolved_then_out_of_range": lambda n: _fill([spec([(0, 0), (1, 1)]), spec([("p", 0)])], n),
}
_names = list(_COND)
for _i, _a in enumerate(_names):
    for _b in _names[_i + 1:]:
        CASES["pair_%s_%s" % (_a, _b)] = _pair(_a, _b)


def random_acyclic(rng, n):
    """A random acyclic case in a random download order: transaction L spends transactions of larger labels only, or
    outside ones; label L stands at position perm[L]."""
    perm = rng.permutation(n)
    specs = [None] * n
    for t in range(n):
        specs[perm[t]] = spec([(int(perm[rng.integers(t + 1, n)]), 0) if t + 1 < n and rng.random() < 0.8 else ("x%d" % t, 0)
                               for _ in range(int(rng.integers(0, 4)))])
    return specs


def all_cases(sizes=SIZES):
    """(name, n) for every case at every size it fits."""
    return [(name, n) for name, build in CASES.items() for n in sizes if build(n) is not None]


def _ext(label) -> bytes:
    return hashlib.sha256(("outside " + label).encode()).digest()


def _claimed_ids(specs, true_ids):
    out = []
    for t, s in enumerate(specs):
        i = bytearray(true_ids[t])
        if "id_mismatch" in s["faults"]:
            i[t % 32] ^= 0x40
        out.append(bytes(i))
    return out


def _inputs(specs, claimed):
    return [[(claimed[r] if isinstance(r, int) else _ext(r), idx) for r, idx in s["inputs"]] for s in specs]


def concrete(specs, ids=None):
    """Plain transactions for resolve_ref and the CPU harness: ids made up (or given), verdicts as the faults say."""
    true_ids = ids or [NC.h32("rid", s["same_as"] if s["same_as"] is not None else t) for t, s in enumerate(specs)]
    claimed = _claimed_ids(specs, true_ids)
    inputs = _inputs(specs, claimed)
    txs = []
    for t, s in enumerate(specs):
        f = s["faults"]
        sigs = [] if "nosig" in f else [(1, 0, 0), (1, 0, 0)]
        if "bad_sig" in f:
            sigs[1] = (0, 0, 0)
        if "bad_key" in f:
            sigs[0] = (0, NC.SIG_BAD_KEY, 0)
        tx = NC.make_tx(("r", t), sigs=sigs, mstatus=1 if "empty" in f else 0,
                        ck=NC._ck_of(sigs, "missing" in f, "malformed" in f))
        tx["recomputed"] = bytes(32) if "empty" in f else true_ids[t]
        tx["claimed"] = claimed[t]
        tx["inputs"], tx["nout"] = inputs[t], s["nout"]
        txs.append(tx)
    return txs


def flatten(txs):
    """The plain transactions as the arrays the lanes read (tests/notarise_cases.flatten + the graph)."""
    f = NC.flatten(txs)
    ins = [x for tx in txs for x in tx["inputs"]]
    f["tx_input_begin"] = np.concatenate([[0], np.cumsum([len(tx["inputs"]) for tx in txs])]).astype(np.uint32)
    f["input_txhash"] = (np.frombuffer(b"".join(h for h, _ in ins), np.uint8).reshape(-1, 32).copy() if ins
                         else np.zeros((0, 32), np.uint8))
    f["input_index"] = np.array([i for _, i in ins], np.uint32)
    f["tx_output_count"] = np.array([tx["nout"] for tx in txs], np.uint32)
    return f


# ---------------------------------------------------------------- real batches (the GPU tests)
def real_leaves(specs):
    """Two leaves a transaction (none for an empty one) -> (leaves, tx_leaf_begin, the true ids as the host hashes
    them: the root over two leaf hashes)."""
    leaves, txb, ids = [], [0], []
    for t, s in enumerate(specs):
        src = s["same_as"] if s["same_as"] is not None else t
        mine = [] if "empty" in s["faults"] else [b"leaf %d/%d " % (src, j) + bytes([src % 251]) * (src % 40) for j in (0, 1)]
        leaves += mine
        txb.append(len(leaves))
        ids.append(hashlib.sha256(b"".join(hashlib.sha256(b).digest() for b in mine)).digest() if mine else bytes(32))
    return leaves, np.array(txb, np.uint32), ids


_SIGNED = {}


def _signed(engine, ids):
    """Two signatures a transaction over its id from a pool of four keys, signed once per distinct batch of ids."""
    key = hashlib.sha256(b"".join(ids)).digest()
    if key not in _SIGNED:
        n = len(ids)
        pool = np.array([np.frombuffer(hashlib.sha256(b"key %d" % k).digest(), np.uint8) for k in range(4)])
        who = (np.arange(2 * n) * 7 // 3) % 4
        tx_of = np.repeat(np.arange(n), 2)
        _SIGNED.clear()                                   # one batch kept: the cases of one size share it
        _SIGNED[key] = engine.sign_batch(pool[who], np.frombuffer(b"".join(ids), np.uint8), (tx_of * 32).astype(np.uint64),
                                         np.full(2 * n, 32, np.uint32))
    pk, sig = _SIGNED[key]
    return pk.copy(), sig.copy()


def real(engine, corpus, specs):
    """-> the keyword arguments of Engine.resolve_batch for the case, with leaves, ids and signatures the engine
    verifies; every fault planted in the data (a flipped signature bit, a key that is not a point, a requirement
    nobody signed, a requirement that is no tree encoding, a flipped id bit, no leaves, no signatures)."""
    from corda_amd import native
    n = len(specs)
    leaves, txb, true_ids = real_leaves(specs)
    claimed = _claimed_ids(specs, true_ids)
    pk, sig = _signed(engine, true_ids)
    bad_keys = corpus["pk"][corpus["status"] == native.CV_SIG_BAD_KEY]
    stranger = np.frombuffer(hashlib.sha256(b"stranger").digest(), np.uint8)
    keep = np.ones(2 * n, bool)
    kind, lkey, rb, trb = [], [], [0], [0]
    for t, s in enumerate(specs):
        f = s["faults"]
        if "bad_sig" in f:
            sig[2 * t + 1, 40] ^= 1
        if "bad_key" in f:
            pk[2 * t] = bad_keys[t % len(bad_keys)]
        if "nosig" in f:
            keep[2 * t:2 * t + 2] = False
        kind.append(native.CV_CK_LEAF), lkey.append(pk[2 * t + 1].copy()), rb.append(len(kind))
        if "missing" in f:
            kind.append(native.CV_CK_LEAF), lkey.append(stranger), rb.append(len(kind))
        if "malformed" in f:
            kind.append(7), lkey.append(np.zeros(32, np.uint8)), rb.append(len(kind))
        trb.append(len(rb) - 1)
    pk, sig = pk[keep], sig[keep]
    tsb = np.concatenate([[0], np.cumsum(keep.reshape(n, 2).sum(1))]).astype(np.uint32)
    nn = len(kind)
    ins = [x for row in _inputs(specs, claimed) for x in row]
    leaf_len = np.array([len(b) for b in leaves], np.uint32)
    leaf_off = np.concatenate([[0], np.cumsum(leaf_len[:-1])]).astype(np.uint64) if leaves else np.zeros(0, np.uint64)
    return dict(arena=np.frombuffer(b"".join(leaves) + bytes(16), np.uint8).copy(), leaf_off=leaf_off, leaf_len=leaf_len,
                tx_leaf_begin=txb, claimed_id=np.frombuffer(b"".join(claimed), np.uint8).reshape(n, 32).copy(),
                sigs=(pk, sig, tsb, None),
                reqs=(np.array(kind, np.uint8), np.array(lkey, np.uint8).reshape(nn, 32), np.zeros(nn, np.int32),
                      np.zeros(nn + 1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.int32), np.array(rb, np.uint32),
                      np.array(trb, np.uint32), pk.copy()),
                tx_input_begin=np.concatenate([[0], np.cumsum([len(s["inputs"]) for s in specs])]).astype(np.uint32),
                input_txhash=(np.frombuffer(b"".join(h for h, _ in ins), np.uint8).reshape(-1, 32).copy() if ins
                              else np.zeros((0, 32), np.uint8)),
                input_index=np.array([i for _, i in ins], np.uint32),
                tx_output_count=np.array([s["nout"] for s in specs], np.uint32))


def components(engine, b):
    """The three component calls on a real batch — cv_merkle_tx_ids_bounded, cv_ed25519_verify_batch over the ids,
    cv_missing_signers — -> (the plain transactions resolve_ref takes, ids, req_missing)."""
    from corda_amd import native
    pk, sig, tsb, _ = b["sigs"]
    n, nsig = len(b["tx_output_count"]), int(tsb[-1])
    ids, mst = engine.merkle_tx_ids(b["arena"], b["leaf_off"], b["leaf_len"], b["tx_leaf_begin"])
    tx_of = np.repeat(np.arange(n), np.diff(tsb))
    bits, sst, bm = np.ones(0, bool), np.zeros(0, np.uint8), None
    if nsig:
        bm, sst = engine.verify_batch(pk, sig, ids.reshape(-1), (tx_of * 32).astype(np.uint64), np.full(nsig, 32, np.uint32))
        bits = native.bitmap_to_bools(bm, nsig)
    req_missing, ck = engine.missing_signers(*b["reqs"], tsb, bitmap=bm)
    tib = b["tx_input_begin"]
    txs = []
    for t in range(n):
        tx = dict(mstatus=int(mst[t]), recomputed=ids[t].tobytes(), claimed=b["claimed_id"][t].tobytes(), tx_pre=0,
                  sigs=[(int(bits[i]), int(sst[i]), 0) for i in range(int(tsb[t]), int(tsb[t + 1]))], ck=int(ck[t]),
                  inputs=[(b["input_txhash"][i].tobytes(), int(b["input_index"][i])) for i in range(int(tib[t]), int(tib[t + 1]))],
                  nout=int(b["tx_output_count"][t]))
        txs.append(tx)
    return txs, ids, req_missing


def same(got, want, what=""):
    """Every output of cv_resolve_batch against resolve_ref's (graph: the words that do not depend on the seed)."""
    for k, w in want.items():
        g = got[k][:G_COMPARED] if k == "graph" else got[k]
        assert np.array_equal(g, w), (what, k, g[:16], w[:16])
