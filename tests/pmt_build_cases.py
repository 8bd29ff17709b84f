"""The partial Merkle tree build cases tests/test_pmt_build.py (CPU) and tests/test_gpu_pmt_build.py (GPU) share, with
the oracle's answer (oracle/merkle_ref.py: get_merkle_tree, build_partial, flatten), computed once per process.

  exhaustive : every include subset of 0..8 distinct leaves, the subset in leaf order: 511 transactions
  random     : 300 trees of 1..70 leaves; every fourth has a repeated leaf, every seventh an absent include, every
               eleventh a repeated include; the include order is shuffled
A batch is a dict of arrays: leaf_hash (nleaves,32), txb u32[ntx+1], include (ninc,32), inc_begin u32[ntx+1],
keep u8[nleaves] (the keep mask that means the same include list, or None where none does) and the expected kind,
left, right, node_hash, tree_begin, ids, status.
"""
import functools
import random

import numpy as np

import merkle_ref as M

OK, EMPTY, NOT_IN_TREE = 0, 1, 3


def expected(leaves, include, base):
    """(status, root, (kind, left, right, hashes)) of one transaction, its nodes numbered from base."""
    try:
        full = M.get_merkle_tree(leaves)
    except M.MerkleTreeException:
        return EMPTY, bytes(32), ([], [], [], [])
    try:
        tree = M.build_partial(full, include)
    except M.MerkleTreeException:
        return NOT_IN_TREE, full.hash, ([], [], [], [])
    return OK, full.hash, M.flatten(tree, base)


def _rows(bs):
    return np.frombuffer(b"".join(bs), np.uint8).reshape(-1, 32).copy()


def batch_of(cases):
    """cases: (leaves, include, keep or None) per transaction -> the batch dict."""
    leaves, incl, keep = [], [], []
    txb, ib, tb = [0], [0], [0]
    kind, left, right, hashes, ids, status = [], [], [], [], [], []
    has_keep = all(c[2] is not None for c in cases)
    for lv, inc, kp in cases:
        st, root, (k, l, r, h) = expected(lv, inc, len(kind))
        kind += k; left += l; right += r; hashes += h
        tb.append(len(kind))
        ids.append(root)
        status.append(st)
        leaves += lv
        incl += inc
        txb.append(len(leaves))
        ib.append(len(incl))
        if has_keep:
            keep += kp
    return {"leaf_hash": _rows(leaves), "txb": np.array(txb, np.uint32), "include": _rows(incl),
            "inc_begin": np.array(ib, np.uint32), "keep": np.array(keep, np.uint8) if has_keep else None,
            "kind": np.array(kind, np.uint8), "left": np.array(left, np.uint32), "right": np.array(right, np.uint32),
            "node_hash": _rows(hashes), "tree_begin": np.array(tb, np.uint32), "ids": _rows(ids),
            "status": np.array(status, np.uint8), "ntx": len(cases)}


@functools.lru_cache(maxsize=None)
def exhaustive_cases():
    out = []
    for n in range(9):
        leaves = [M.sha256(bytes([n, i])) for i in range(n)]
        for mask in range(1 << n):
            keep = [(mask >> i) & 1 for i in range(n)]
            out.append((leaves, [leaves[i] for i in range(n) if keep[i]], keep))
    assert len(out) == 511
    return tuple(out)


@functools.lru_cache(maxsize=None)
def random_cases():
    rng = random.Random(20161)
    out = []
    for t in range(300):
        n = rng.randint(1, 70)
        leaves = [M.sha256(rng.randbytes(8)) for _ in range(n)]
        if t % 4 == 0 and n > 1:
            a, b = rng.sample(range(n), 2)
            leaves[a] = leaves[b]
        include = [h for h in leaves if rng.random() < 0.3]
        if t % 7 == 0:
            include.append(M.sha256(b"absent" + bytes([t % 256])))
        if t % 11 == 0 and include:
            include.append(rng.choice(include))
        rng.shuffle(include)
        out.append((leaves, include, None))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def random_keep_cases():
    """The random trees again with a keep mask as the include source: include = the kept leaves' hashes."""
    rng = random.Random(20162)
    out = []
    for leaves, _, _ in random_cases():
        keep = [1 if rng.random() < 0.3 else 0 for _ in leaves]
        out.append((leaves, [h for h, k in zip(leaves, keep) if k], keep))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def exhaustive_batch():
    return batch_of(exhaustive_cases())


@functools.lru_cache(maxsize=None)
def random_batch():
    return batch_of(random_cases())


@functools.lru_cache(maxsize=None)
def random_keep_batch():
    return batch_of(random_keep_cases())


@functools.lru_cache(maxsize=None)
def full_batch():
    """The 811 transactions of the GPU test: exhaustive, then random."""
    return batch_of(exhaustive_cases() + random_cases())


def hashed_abcdef():
    """The reference's test leaves (PartialMerkleTreeTest.kt:23-26), as tests/test_partial_merkle.py::_hashed."""
    return [M.sha256(bytes([7, 0, ord(c)])) for c in "abcdef"]


def reference_scenarios():
    """The build scenarios of PartialMerkleTreeTest.kt:88-120 and the five-leaf build of its duplicate-leaf test:
    (name, leaves, include, expected status)."""
    h = hashed_abcdef()
    aaa = [h[0]] * 3
    return [("only left nodes branch :89-94", h, [h[3], h[5]], OK),
            ("include zero leaves :96-100", h, [], OK),
            ("include all leaves :102-106", h, list(h), OK),
            ("duplicate leaves failure :108-112", h, [h[3], h[5], h[3], h[5]], NOT_IN_TREE),
            ("only duplicate leaves, less included :114-120", aaa, aaa[:1], NOT_IN_TREE),
            ("five leaves, a DuplicatedLeaf on two levels", h[:5], [h[3], h[4]], OK)]
