"""Cases of the missing-signers feature (cv_missing_signers; corda_amd/csrc/cv_ck.h), shared by tests/test_ck_cpu.py
(the per-lane core on the CPU) and tests/test_gpu_ck.py (the kernels), with the oracle they are compared with.

fulfilled_ref restates CompositeKey.isFulfilledBy of the reference literally (core/src/main/kotlin/net/corda/core/
crypto/CompositeKey.kt:49 for a Leaf, :75-81 for a Node) with Kotlin's Int sum, which wraps at 32 bits — where the
mirror's crypto.CompositeKey.is_fulfilled_by, summing in unbounded integers, differs.  A case is a list of
transactions (must_sign trees, signer keys, allowed requirements) with an optional verdict bitmap and an optional
mutation of the flat arrays that makes one requirement malformed; expect() gives req_missing and tx_status by the rule of
include/cordaverify.h.  Every comparison is exact.

Reference tests restated: CompositeKeyTests.kt:22-49, TransactionTests.kt:25-58.
"""
import hashlib
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np

from corda_amd.crypto import CompositeKey, EdDSAPublicKey

LEAF, NODE = 0, 1
FULFILLED, MISSING, MALFORMED = 0, 1, 2
VS_OK, VS_BAD_SIGNATURE, VS_MISSING, VS_MALFORMED = 0, 1, 2, 3
WIDE_MINS = (0, 1, 0xFFFFFFFF)          # the default, always the wave path, never
TILE = 64                               # CV_CK_TILE (test_ck_cpu.py checks it against the header)
Leaf, Node = CompositeKey.Leaf, CompositeKey.Node


def _i32(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def fulfilled_ref(key, sig_keys) -> bool:
    """CompositeKey.isFulfilledBy(keys), CompositeKey.kt:49 and :75-81, the sum a Kotlin Int."""
    if isinstance(key, Leaf):
        return key.public_key in sig_keys                          # publicKey in keys
    total = 0
    for i, child in enumerate(key.children):                       # children.mapIndexed { ... }.sum()
        total = _i32(total + (key.weights[i] if fulfilled_ref(child, sig_keys) else 0))
    return total >= key.threshold


def key(tag, i=0) -> EdDSAPublicKey:
    return EdDSAPublicKey(hashlib.sha256(f"ck-{tag}-{i}".encode()).digest())


def leaf(tag, i=0) -> CompositeKey:
    return Leaf(key(tag, i))


def node(threshold, children, weights=None) -> CompositeKey:
    return Node(threshold, list(children), [1] * len(children) if weights is None else list(weights))


@dataclass
class Tx:
    must_sign: List[CompositeKey]
    signers: List[EdDSAPublicKey]
    allowed: List[CompositeKey] = field(default_factory=list)


@dataclass
class Case:
    txs: List[Tx]
    bitmap: Optional[Callable[[int], np.ndarray]] = None      # nsig -> uint64 words
    mutate: Optional[Callable[[Dict[str, np.ndarray]], Dict[int, int]]] = None   # flat arrays -> {requirement: 2}
    overflows: bool = False                                   # the mirror's unbounded sum differs here


def flatten(txs: List[Tx]) -> Dict[str, np.ndarray]:
    """The flat encoding of include/cordaverify.h; a subtree OBJECT met twice inside one requirement is shared."""
    kind, keys, thr, cb, child, weight, rb, trb, tsb, sig, allowed = [], [], [], [0], [], [], [0], [0], [0], [], []

    def emit(k, seen):
        if id(k) in seen:
            return seen[id(k)]
        if isinstance(k, Leaf):
            kind.append(LEAF); keys.append(k.public_key.encoded); thr.append(0)
        else:
            idx = [emit(c, seen) for c in k.children]
            kind.append(NODE); keys.append(bytes(32)); thr.append(k.threshold)
            child.extend(idx); weight.extend(k.weights)
        cb.append(len(child))
        seen[id(k)] = len(kind) - 1
        return len(kind) - 1

    for tx in txs:
        for r in tx.must_sign:
            emit(r, {})
            rb.append(len(kind))
            allowed.append(1 if r in tx.allowed else 0)
        trb.append(len(rb) - 1)
        sig.extend(k.encoded for k in tx.signers)
        tsb.append(len(sig))
    return {"kind": np.array(kind, np.uint8), "leaf_key": np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32).copy(),
            "threshold": np.array(thr, np.int32), "child_begin": np.array(cb, np.uint32),
            "child": np.array(child, np.uint32), "weight": np.array(weight, np.int32),
            "req_begin": np.array(rb, np.uint32), "tx_req_begin": np.array(trb, np.uint32),
            "sig_key": np.frombuffer(b"".join(sig), np.uint8).reshape(-1, 32).copy(),
            "tx_sig_begin": np.array(tsb, np.uint32), "req_allowed": np.array(allowed, np.uint8)}


def build(case: Case):
    """(flat arrays incl. req_allowed and bitmap or None, expected req_missing, expected tx_status)."""
    f = flatten(case.txs)
    nsig = int(f["tx_sig_begin"][-1])
    f["bitmap"] = None if case.bitmap is None else np.ascontiguousarray(case.bitmap(nsig), np.uint64)
    bad = case.mutate(f) if case.mutate else {}
    bits = None if f["bitmap"] is None else np.unpackbits(f["bitmap"].view(np.uint8), bitorder="little")
    req_missing, tx_status = [], []
    r = 0
    for t, tx in enumerate(case.txs):
        sig_keys = set(tx.signers)
        mine = []
        for req in tx.must_sign:
            mine.append(bad.get(r, FULFILLED if fulfilled_ref(req, sig_keys) else MISSING))
            r += 1
        sb, se = int(f["tx_sig_begin"][t]), int(f["tx_sig_begin"][t + 1])
        if MALFORMED in mine:
            st = VS_MALFORMED
        elif sb == se or (bits is not None and not bits[sb:se].all()):
            st = VS_BAD_SIGNATURE
        elif any(m == MISSING and req not in tx.allowed for m, req in zip(mine, tx.must_sign)):
            st = VS_MISSING
        else:
            st = VS_OK
        req_missing += mine
        tx_status.append(st)
    return f, np.array(req_missing, np.uint8), np.array(tx_status, np.uint8)


def all_ones(nsig):
    return np.full((nsig + 63) // 64, 0xFFFFFFFFFFFFFFFF, np.uint64)


def ones_except(*zero_bits, tail_zero=True):
    def make(nsig):
        w = all_ones(nsig)
        if tail_zero and nsig % 64:
            w[-1] = np.uint64((1 << (nsig % 64)) - 1)
        for b in zero_bits:
            if b < 64 * len(w):
                w[b // 64] &= np.uint64(~(1 << (b % 64)) & 0xFFFFFFFFFFFFFFFF)
        return w
    return make


# ---------------------------------------------------------------- the reference's own tests
A, B, Ch = leaf("alice"), leaf("bob"), leaf("charlie")
a, b, c = A.public_key, B.public_key, Ch.public_key


def composite_key_tests():
    a_or_b, a_and_b = node(1, [A, B]), node(2, [A, B])
    ab_or_c = node(1, [node(2, [A, B]), Ch])
    txs = []
    for req, signers in ((A, [a]), (a_or_b, [b]), (a_and_b, [a, b]), (ab_or_c, [a, b])):
        txs.append(Tx([req], signers))
        for i in range(len(signers)):                            # each with a signer removed (one stays where two were;
            rest = signers[:i] + signers[i + 1:]                 # where one was, a stranger signs)
            txs.append(Tx([req], rest or [key("stranger")]))
    txs.append(Tx([ab_or_c], [c]))
    return Case(txs)


def transaction_tests():
    k1, k2, issuer = leaf("dummy", 1), leaf("dummy", 2), key("issuer")
    ms = [k1, k2]
    return Case([Tx(ms, [k2.public_key]), Tx(ms, [k1.public_key]), Tx(ms, [issuer], [k1]),
                 Tx(ms, [k1.public_key], [k2]), Tx(ms, [k2.public_key], [k1]), Tx(ms, [k1.public_key, k2.public_key]),
                 Tx(ms, [issuer]), Tx(ms, [issuer], [k1, k2])])


# ---------------------------------------------------------------- weights and thresholds
def weights_thresholds():
    five = [leaf("w", i) for i in range(5)]
    k = [x.public_key for x in five]
    three_of_five = node(6, five, [1, 2, 3, 4, 5])
    neg = node(2, [leaf("w", 0), leaf("w", 1), leaf("w", 2)], [2, 1, -2])
    return Case([
        Tx([three_of_five], [k[0], k[1], k[2]]),                 # 1 + 2 + 3 = 6
        Tx([three_of_five], [k[0], k[1], k[3]]),                 # 7
        Tx([three_of_five], [k[0], k[4]]),                       # 6 with two signers
        Tx([three_of_five], [k[0], k[1]]),                       # 3: missing
        Tx([three_of_five], [k[4]]),                             # 5: missing
        Tx([node(0, [leaf("w", 0)])], [key("nobody")]),          # thresholds 0 and -1: nobody's signature fulfils them
        Tx([node(-1, [leaf("w", 0)])], [key("nobody")]),
        Tx([node(0, [leaf("w", 0)]), node(-1, [leaf("w", 1)])], []),      # ... and with no signer at all
        Tx([node(1, [])], [k[0]]),                               # childless: fulfilled iff threshold <= 0
        Tx([node(0, [])], [k[0]]),
        Tx([neg], [k[0], k[1]]),                                 # 3 >= 2
        Tx([neg], [k[0], k[1], k[2]]),                           # the negative weight takes 3 down to 1: missing
        Tx([node(-3, [leaf("w", 0)], [-5])], [k[0]]),            # -5 < -3: missing
        Tx([node(-3, [leaf("w", 0)], [-5])], [k[1]]),            # 0 >= -3
    ])


def overflow():
    four = [leaf("o", i) for i in range(4)]
    k = [x.public_key for x in four]
    big = node(1, four, [1 << 30] * 4)
    return Case([Tx([big], k),                                   # 4 x 2^30 wraps to 0 < 1: missing
                 Tx([big], k[:3]),                               # 3 x 2^30 wraps negative: missing
                 Tx([big], k[:1]),                               # 2^30: fulfilled
                 Tx([node(-(1 << 31), four, [1 << 30] * 4)], k[:2])],   # 2^31 wraps to Int.MIN_VALUE >= itself
                overflows=True)


# ---------------------------------------------------------------- structure
def structure():
    x, y, z = leaf("s", 0), leaf("s", 1), leaf("s", 2)
    kx, ky, kz = x.public_key, y.public_key, z.public_key
    twice = node(2, [x, x])                                      # the same object: one node, listed twice
    shared = node(2, [x, y])
    two_parents = node(2, [node(1, [shared, z]), node(1, [shared])])
    chain = x
    for _ in range(12):
        chain = node(1, [chain])
    return Case([
        Tx([twice], [kx]), Tx([twice], [ky]),
        Tx([node(2, [leaf("s", 0), leaf("s", 0)])], [kx]),       # equal but distinct objects: two nodes
        Tx([two_parents], [kx, ky]), Tx([two_parents], [kx, kz]), Tx([two_parents], [kz]),
        Tx([chain], [kx]), Tx([chain], [ky]),
        Tx([x, y], [kx, kx, kx]),                                # duplicate signer keys
        Tx([node(2, [x, y])], [kx, kx]),
        Tx([y, y, leaf("s", 1)], [kx]),                          # equal requirements are each flagged
        Tx([y, y], [ky], [y]),
        Tx([], [kx]),                                            # no requirements: never missing
        Tx([], []),                                              # ... and no signers: bad signature
        Tx([x], []), Tx([x, node(0, [])], []),                   # no signers
    ])


def key_compares():
    base = key("cmp").encoded
    near = [EdDSAPublicKey(base[:n] + bytes(v ^ 0x5A for v in base[n:])) for n in (4, 16, 31)]
    last_byte = EdDSAPublicKey(base[:31] + bytes([base[31] ^ 0x80]))
    first_byte = EdDSAPublicKey(bytes([base[0] ^ 1]) + base[1:])
    others = [key("cmp-other", i) for i in range(9)]
    req = Leaf(EdDSAPublicKey(base))
    txs = [Tx([req], [n]) for n in near] + [Tx([req], [last_byte]), Tx([req], [first_byte]), Tx([req], near + [last_byte])]
    txs += [Tx([req, Leaf(near[0]), Leaf(near[2])], near[:1] + others[:3]),
            Tx([req], others + [EdDSAPublicKey(base)]),          # a match only in the last signer
            Tx([req], [EdDSAPublicKey(base)] + others),          # ... only in the first
            Tx([req], others)]
    return Case(txs)


def req_allowed():
    x, y = leaf("al", 0), leaf("al", 1)
    kx, ky = x.public_key, y.public_key
    return Case([Tx([x], [ky], [x]),                             # allowed and missing
                 Tx([x], [kx], [x]),                             # allowed and fulfilled
                 Tx([x, y], [key("al", 9)], [x]),                # one of two missing requirements allowed
                 Tx([x, y], [key("al", 9)], [x, y]),
                 Tx([node(2, [x, y])], [kx], [node(2, [leaf("al", 0), leaf("al", 1)])]),   # structural equality
                 Tx([x, y], [key("al", 9)], [leaf("al", 7)])])


# ---------------------------------------------------------------- bitmap
def _bitmap_txs(end):
    """Three transactions with signatures [0, 3), [3, end), [end, end + 3), each signed by what it needs."""
    txs = []
    for j, n in enumerate((3, end - 3, 3)):
        ks = [key(f"bm{end}-{j}", i) for i in range(n)]
        txs.append(Tx([Leaf(ks[0]), node(2, [Leaf(ks[0]), Leaf(ks[-1])])], ks))
    return txs


def bitmap_cases():
    out = {}
    for end in (63, 64, 65):
        out[f"bitmap_end{end}_first"] = Case(_bitmap_txs(end), bitmap=ones_except(3))
        out[f"bitmap_end{end}_last"] = Case(_bitmap_txs(end), bitmap=ones_except(end - 1))
        # 0 bits just outside the middle range: its neighbours fail, it does not
        out[f"bitmap_end{end}_outside"] = Case(_bitmap_txs(end), bitmap=ones_except(2, end))
    # every bit at and above nsig set or clear: neither matters
    out["bitmap_tail_ones"] = Case(_bitmap_txs(65), bitmap=lambda nsig: all_ones(nsig))
    out["bitmap_all_zero"] = Case(_bitmap_txs(64) + [Tx([leaf("bz")], [])], bitmap=lambda nsig: np.zeros((nsig + 63) // 64, np.uint64))
    return out


# ---------------------------------------------------------------- malformed
def _malformed(mutation):
    """A malformed transaction (one requirement: a 2-of-2 Node over two Leaves, nodes 3..5, children entries 2..3)
    between two well-formed ones, each of which begins with a Leaf and holds a Node."""
    def txs():
        out = []
        for j in range(3):
            x, y = leaf(f"mal{j}", 0), leaf(f"mal{j}", 1)
            out.append(Tx([node(2, [x, y])], [x.public_key, y.public_key] if j != 2 else [x.public_key]))
        return out

    def mutate(f):
        assert f["req_begin"].tolist() == [0, 3, 6, 9] and f["child_begin"].tolist() == [0, 0, 0, 2, 2, 2, 4, 4, 4, 6]
        mutation(f)
        return {1: MALFORMED}
    return Case(txs(), mutate=mutate)


def _set(name, index, value):
    def m(f):
        f[name][index] = value
    return m


def malformed_cases():
    out = {
        "malformed_child_is_self": _malformed(_set("child", 3, 5)),
        "malformed_child_in_previous_requirement": _malformed(_set("child", 2, 2)),
        "malformed_kind_3": _malformed(_set("kind", 4, 3)),
        "malformed_kind_3_root": _malformed(_set("kind", 5, 3)),
        "malformed_descending_range": _malformed(_set("child_begin", 6, 1)),
        "malformed_range_past_nchild": _malformed(_set("child_begin", 6, 7)),
        "malformed_child_far_away": _malformed(_set("child", 2, 0xFFFFFFFF)),
    }
    # an empty requirement: the middle transaction's one entry is flattened as a placeholder Leaf, which the mutation
    # takes out again, so its requirement becomes nodes [3, 3); the right neighbour owns two requirements
    x0, y0, x1, y1, x2 = leaf("e0", 0), leaf("e0", 1), leaf("e1", 0), leaf("e1", 1), leaf("e2", 0)
    txs = [Tx([node(2, [x0, y0])], [x0.public_key, y0.public_key]), Tx([leaf("e-empty")], [x1.public_key]),
           Tx([node(2, [x1, y1]), node(1, [x2, leaf("e2", 1)])], [x1.public_key, x2.public_key])]

    def empty(f):
        # drop the placeholder Leaf (node 3) of the middle transaction: its requirement becomes [3, 3)
        for name in ("kind", "threshold"):
            f[name] = np.delete(f[name], 3)
        f["leaf_key"] = np.delete(f["leaf_key"], 3, axis=0)
        f["child_begin"] = np.delete(f["child_begin"], 4)
        f["child"] = np.where(f["child"] > 3, f["child"] - 1, f["child"]).astype(np.uint32)
        f["req_begin"] = np.where(f["req_begin"] > 3, f["req_begin"] - 1, f["req_begin"]).astype(np.uint32)
        assert f["req_begin"].tolist() == [0, 3, 3, 6, 9]
        return {1: MALFORMED}
    out["malformed_empty_requirement"] = Case(txs, mutate=empty)
    return out


# ---------------------------------------------------------------- batch sizes and wide shapes
def _small_shapes(n, seed):
    rng = np.random.default_rng(seed)
    pool = [key("pool", i) for i in range(12)]
    txs = []
    for t in range(n):
        shape = t % 6
        ks = [pool[int(i)] for i in rng.choice(12, 4, replace=False)]
        signers = [ks[int(i)] for i in rng.choice(4, int(rng.integers(0, 4)), replace=False)]
        if shape == 0:
            ms = [Leaf(ks[0])]
        elif shape == 1:                                         # the notary shape: three entries, one a 1-of-2 node
            ms = [Leaf(ks[0]), Leaf(ks[1]), node(1, [Leaf(ks[2]), Leaf(ks[3])])]
        elif shape == 2:
            ms = [node(2, [Leaf(ks[0]), node(1, [Leaf(ks[1]), Leaf(ks[2])])])]
        elif shape == 3:
            ms = []
        elif shape == 4:
            ms = [node(3, [Leaf(k) for k in ks], [1, 1, 2, 2]), Leaf(ks[3])]
        else:
            ms = [Leaf(k) for k in ks]
        txs.append(Tx(ms, signers, [ms[0]] if ms and t % 4 == 0 else []))
    return txs


def batch(n):
    return lambda: Case(_small_shapes(n, n), bitmap=None if n % 2 else ones_except(*range(0, 2 * n, 7)))


def wide_shapes():
    """Signer counts T-1, T, T+1, 2T+1 x Leaf counts 63, 64, 65, 129 x the one matching key in the last key of the
    last tile, in the first key, nowhere: an any-of and an all-of Node over the leaves, and the matching Leaf alone."""
    txs = []
    n = 0
    for ns in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        for nl in (63, 64, 65, 129):
            for where in ("last", "first", "none"):
                n += 1
                leaves = [leaf(f"wl{n}", i) for i in range(nl)]
                signers = [key(f"ws{n}", i) for i in range(ns)]
                hit = leaves[nl - 1] if n % 2 else leaves[(7 * n) % nl]
                if where != "none":
                    signers[ns - 1 if where == "last" else 0] = hit.public_key
                txs.append(Tx([node(1, leaves), node(nl, leaves), hit], signers))
    return Case(txs)


def outlier():
    """A 300-leaf x 300-signer transaction (300 Leaf requirements, every other one signed for, and an all-of Node
    over the signed ones) next to one-leaf transactions."""
    leaves = [leaf("big", i) for i in range(300)]
    signers = [leaves[(i * 7) % 300].public_key if i % 2 == 0 else key("big-stranger", i) for i in range(300)]
    signed = [leaves[(i * 7) % 300] for i in range(0, 300, 2)]
    small = [Tx([leaf("sm", i)], [key("sm", i if i % 2 else 99)]) for i in range(5)]
    return Case(small[:3] + [Tx(leaves + [node(len(signed), signed), node(len(signed) + 1, signed + [leaves[1]])], signers,
                                [leaves[1]])] + small[3:])


CASES: Dict[str, Callable[[], Case]] = {
    "composite_key_tests": composite_key_tests, "transaction_tests": transaction_tests,
    "weights_thresholds": weights_thresholds, "overflow": overflow, "structure": structure,
    "key_compares": key_compares, "req_allowed": req_allowed,
    **{k: (lambda v=v: v) for k, v in bitmap_cases().items()},
    **{k: (lambda v=v: v) for k, v in malformed_cases().items()},
    **{f"batch_{n}": batch(n) for n in (1, 63, 64, 65, 255, 256, 257)},
    "wide_shapes": wide_shapes, "outlier_300x300": outlier,
}


def no_requirements() -> Case:
    """Transactions none of which has a requirement (nreq = nnodes = nchild = 0: every node-sized piece of the call's
    buffer is empty): with signers nothing is missing, without any the status is bad signature.  Not in CASES: the
    tests over CASES assume at least one node."""
    return Case([Tx([], [key("nr", 0)]), Tx([], []), Tx([], [key("nr", 1), key("nr", 2)])])


def mirror_agrees(case: Case) -> bool:
    """fulfilled_ref == crypto.CompositeKey.is_fulfilled_by on every requirement of the case."""
    return all(fulfilled_ref(r, set(tx.signers)) == r.is_fulfilled_by(set(tx.signers)) for tx in case.txs for r in tx.must_sign)
