"""PartialMerkleTree.build / FilteredTransaction.buildMerkleTransaction on the GPU (cv_partial_merkle_build,
cv_filtered_build: the kernels of corda_amd/csrc/cv_k_pmt.hip through the C-ABI) against the oracle
(oracle/merkle_ref.py) and the host mirror, and fed unchanged into cv_partial_merkle_verify.
"""
import hashlib
import random

import numpy as np
import pytest

import merkle_ref as M
import pmt_build_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built(engine):
    """ONE cv_partial_merkle_build call over the 511 exhaustive + 300 random transactions (four workgroups, the last
    ragged; transactions with no leaves and with failing includes among them)."""
    b = C.full_batch()
    assert b["ntx"] == 811
    return b, engine.partial_merkle_build(b["leaf_hash"], b["txb"], b["include"], b["inc_begin"])


def test_batch_equals_oracle(built):
    b, got = built
    assert (b["status"] == C.EMPTY).sum() == 1 and (b["status"] == C.NOT_IN_TREE).sum() >= 40
    for name, a in zip(("kind", "left", "right", "node_hash", "tree_begin", "ids", "status"), got):
        assert a.shape == b[name].shape and np.array_equal(a, b[name]), name


def test_batch_feeds_verify_unchanged(engine, built):
    """The build's output arrays as cv_partial_merkle_verify's input, ids as the roots, the include lists as the
    check lists: verdict 1 for every built tree whose include list is its included leaves — every one but those the
    reference's count rule lets through although the list is not the included leaves (a leaf carried twice and
    listed once beside an absent or a twice-listed hash: as many used as listed), where the oracle's verify says 0
    too."""
    b, (kind, left, right, node_hash, tb, ids, st) = built
    v, vst = engine.partial_merkle_verify(kind, left, right, node_hash, tb, ids, b["include"], b["inc_begin"])
    ok = st == C.OK
    assert np.array_equal(vst[ok], np.zeros(ok.sum(), np.uint8)) and np.array_equal(vst[~ok], np.full((~ok).sum(), 2, np.uint8))
    want = np.zeros(b["ntx"], np.uint8)
    hashes = [h.tobytes() for h in node_hash]
    for t in np.flatnonzero(ok):
        lo, hi = int(b["inc_begin"][t]), int(b["inc_begin"][t + 1])
        want[t] = M.verify_flat(kind, left, right, hashes, int(tb[t]), int(tb[t + 1]), ids[t].tobytes(),
                                [b["include"][j].tobytes() for j in range(lo, hi)])[0]
    assert np.array_equal(v, want)
    assert v[:511].sum() == 510                                   # every exhaustive tree
    # from the inputs alone: the include list is, as a multiset, the leaves whose hash it names
    clean = np.zeros(b["ntx"], bool)
    for t in range(b["ntx"]):
        inc = sorted(b["include"][j].tobytes() for j in range(int(b["inc_begin"][t]), int(b["inc_begin"][t + 1])))
        leaves = [b["leaf_hash"][i].tobytes() for i in range(int(b["txb"][t]), int(b["txb"][t + 1]))]
        clean[t] = inc == sorted(h for h in leaves if h in set(inc))
    assert np.array_equal(v[ok & clean], np.ones((ok & clean).sum(), np.uint8)) and (ok & clean).sum() > 600
    # (the ids against the Merkle id kernels: test_ids_equal_merkle_tx_ids, where the leaves are blobs both calls hash)
    assert np.array_equal(ids, b["ids"])


@pytest.mark.parametrize("ntx", [1, 3])
def test_transactions_without_leaves_alone(engine, ntx):
    """A batch with no leaf and no include at all: the build emits no node (every leaf-, include- and node-sized piece
    of its buffer is empty), and cv_partial_merkle_verify over that output runs with nnodes = 0 and ncheck = 0."""
    b = C.batch_of([([], [], None)] * ntx)
    assert b["status"].tolist() == [C.EMPTY] * ntx and b["kind"].size == 0 and b["tree_begin"].tolist() == [0] * (ntx + 1)
    got = engine.partial_merkle_build(b["leaf_hash"], b["txb"], b["include"], b["inc_begin"])
    for name, a in zip(("kind", "left", "right", "node_hash", "tree_begin", "ids", "status"), got):
        assert a.shape == b[name].shape and np.array_equal(a, b[name]), name
    kind, left, right, node_hash, tb, ids, _ = got
    v, vst = engine.partial_merkle_verify(kind, left, right, node_hash, tb, ids, b["include"], b["inc_begin"])
    want = [M.verify_flat([], [], [], [], 0, 0, bytes(32), [])] * ntx         # (0, 2): no nodes are no tree encoding
    assert list(zip(v.tolist(), vst.tolist())) == want


def test_ids_equal_merkle_tx_ids(engine):
    """cv_filtered_build's ids = cv_merkle_tx_ids_ex over the same leaf blobs (no-leaf transactions included)."""
    rng = random.Random(5)
    blobs, begin = [], [0]
    for t in range(200):
        blobs += [rng.randbytes(rng.randint(1, 300)) for _ in range(0 if t % 50 == 7 else rng.randint(1, 12))]
        begin.append(len(blobs))
    lens = np.array([len(x) for x in blobs], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    arena = np.frombuffer(b"".join(blobs) + bytes(16), np.uint8)
    keep = np.array([rng.random() < 0.4 for _ in blobs], np.uint8)
    out = engine.filtered_build(arena, offs, lens, np.array(begin, np.uint32), keep)
    ids, st = engine.merkle_tx_ids(arena, offs, lens, np.array(begin, np.uint32))
    assert np.array_equal(out[5], ids) and np.array_equal(out[6] == C.EMPTY, st == 1) and (st == 1).sum() == 4
    want = C.batch_of([([hashlib.sha256(x).digest() for x in blobs[begin[t]:begin[t + 1]]],
                        [hashlib.sha256(blobs[i]).digest() for i in range(begin[t], begin[t + 1]) if keep[i]], None)
                       for t in range(200)])
    for name, a in zip(("kind", "left", "right", "node_hash", "tree_begin", "ids", "status"), out):
        assert np.array_equal(a, want[name]), name


def test_deep_tree_single_and_empty_batches_and_short_capacity(engine):
    """One transaction of 1,025 leaves with three scattered includes (twelve levels, a DuplicatedLeaf on ten of them);
    ntx = 1 and ntx = 0; nodes_cap one short of the total: CV_E_ARGS with *nnodes, tree_begin, status and ids set."""
    import ctypes
    from corda_amd import native
    leaves = [M.sha256(b"deep" + i.to_bytes(2, "big")) for i in range(1025)]
    inc = [leaves[1024], leaves[3], leaves[700]]
    b = C.batch_of([(leaves, inc, None)])
    got = engine.partial_merkle_build(b["leaf_hash"], b["txb"], b["include"], b["inc_begin"])
    for name, a in zip(("kind", "left", "right", "node_hash", "tree_begin", "ids", "status"), got):
        assert np.array_equal(a, b[name]), name
    nn = int(b["tree_begin"][1])
    assert native.partial_merkle_build_bound(b["txb"]) == 2069 and nn == len(b["kind"]) > 3   # 2,059 entries + 10
    # all 1,025 included: exactly the bound
    full = C.batch_of([(leaves, leaves, None)])
    got = engine.partial_merkle_build(full["leaf_hash"], full["txb"], full["include"], full["inc_begin"])
    assert got[4].tolist() == [0, 2069] and np.array_equal(got[1], full["left"]) and np.array_equal(got[0], full["kind"])
    # ntx = 0
    e = engine.partial_merkle_build(np.zeros((0, 32), np.uint8), [0], np.zeros((0, 32), np.uint8), [0])
    assert [a.shape[0] for a in e] == [0, 0, 0, 0, 1, 0, 0]
    # a capacity one short: through the binding a ValueError naming the count, through the C-ABI CV_E_ARGS
    with pytest.raises(ValueError, match=str(nn)):
        engine.partial_merkle_build(b["leaf_hash"], b["txb"], b["include"], b["inc_begin"], nodes_cap=nn - 1)
    p = native._p
    kind, left, right = np.full(nn, 0xEE, np.uint8), np.zeros(nn, np.uint32), np.zeros(nn, np.uint32)
    hashes, tb, ids, st = np.zeros((nn, 32), np.uint8), np.zeros(2, np.uint32), np.zeros((1, 32), np.uint8), np.full(1, 9, np.uint8)
    cnt = ctypes.c_size_t(0)
    rc = engine._lib.cv_partial_merkle_build(engine._h, 1, p(b["leaf_hash"]), p(b["txb"]), p(b["include"]), p(b["inc_begin"]),
                                             nn - 1, p(kind), p(left), p(right), p(hashes), p(tb), p(ids), p(st),
                                             ctypes.byref(cnt))
    assert rc == -3 and cnt.value == nn and tb.tolist() == [0, nn] and st[0] == 0 and np.array_equal(ids, b["ids"])
    assert (kind == 0xEE).all()                                   # the node arrays were left alone
    rc = engine._lib.cv_partial_merkle_build(engine._h, 1, p(b["leaf_hash"]), p(b["txb"]), p(b["include"]), p(b["inc_begin"]),
                                             nn, p(kind), p(left), p(right), p(hashes), p(tb), None, p(st), ctypes.byref(cnt))
    assert rc == 0 and np.array_equal(kind, b["kind"]) and np.array_equal(hashes, b["node_hash"])   # ids optional


def _wire_transactions():
    """300 WireTransactions shaped as tests/test_partial_merkle.py::test_gpu_filtered_transactions."""
    from corda_amd.transactions import WireTransaction
    rng = random.Random(9)
    return [WireTransaction(inputs=[rng.randbytes(rng.randint(30, 120)) for _ in range(rng.randint(0, 3))],
                            outputs=[rng.randbytes(rng.randint(100, 600)) for _ in range(rng.randint(1, 4))],
                            attachments=[rng.randbytes(32) for _ in range(rng.randint(0, 2))],
                            commands=[rng.randbytes(rng.randint(50, 300)) for _ in range(rng.randint(1, 3))])
            for _ in range(300)]


def test_filtered_build_equals_host_mirror(engine):
    from corda_amd.transactions import (FilteredTransaction, MerkleTreeException, WireTransaction, build_filtered_batch,
                                        compute_ids, verify_filtered_batch)
    wtxs = _wire_transactions()
    keep_cmd = lambda b: b[0] % 2 == 0  # noqa: E731
    ftxs, ids = build_filtered_batch(wtxs, (None, lambda b: True, None, keep_cmd), engine)
    fresh = _wire_transactions()
    want_ids = compute_ids(fresh, engine)
    assert ids == want_ids and len(ftxs) == 300
    for wtx, ftx in zip(fresh, ftxs):
        host = FilteredTransaction.build_merkle_transaction(wtx, filter_outputs=lambda b: True, filter_commands=keep_cmd)
        assert ftx.partial_merkle_tree.flatten() == host.partial_merkle_tree.flatten()
        assert ftx.filtered_leaves.get_filtered_hashes() == host.filtered_leaves.get_filtered_hashes()
    assert verify_filtered_batch(list(zip(ftxs, ids)), engine) == [True] * 300
    # two equal leaves of which one is kept: the kept hash sits on two leaves against a list of one
    twin = WireTransaction(inputs=[b"same leaf bytes" * 3], outputs=[b"same leaf bytes" * 3, b"another output" * 5])
    per_tx = [(lambda b: True, None, None, None), (None, lambda b: True, None, None)]
    res, rid = build_filtered_batch([twin, wtxs[0]], per_tx, engine, raise_first=False)
    assert isinstance(res[0], MerkleTreeException) and str(res[0]) == "Some of the provided hashes are not in the tree."
    assert isinstance(res[1], FilteredTransaction) and rid[0] == compute_ids([twin], engine)[0]
    with pytest.raises(MerkleTreeException, match="not in the tree"):
        build_filtered_batch([twin], per_tx[0], engine)
    with pytest.raises(MerkleTreeException, match="not in the tree"):
        FilteredTransaction.build_merkle_transaction(twin, filter_inputs=lambda b: True)     # as the host mirror


def test_mirror_build_partial_trees(engine):
    """The reference's build scenarios through build_partial_trees, with the reference's exceptions."""
    from corda_amd.transactions import MerkleTree, MerkleTreeException, PartialMerkleTree, SecureHash, build_partial_trees
    sh = lambda hs: [SecureHash(h) for h in hs]  # noqa: E731
    sc = C.reference_scenarios()
    res = build_partial_trees([(sh(lv), sh(inc)) for _, lv, inc, _ in sc], engine, raise_first=False)
    for (name, lv, inc, st), r in zip(sc, res):
        if st == C.OK:
            host = PartialMerkleTree.build(MerkleTree.get_merkle_tree(sh(lv)), sh(inc))
            assert r.flatten() == host.flatten() == M.flatten(M.build_partial(M.get_merkle_tree(lv), inc)), name
            assert r.verify(MerkleTree.get_merkle_tree(sh(lv)).hash, sh(inc), engine), name
        else:
            assert isinstance(r, MerkleTreeException) and str(r) == "Some of the provided hashes are not in the tree.", name
    h = C.hashed_abcdef()
    with pytest.raises(MerkleTreeException, match="Some of the provided hashes are not in the tree."):
        build_partial_trees([(sh(h), sh([h[3], h[5]])), (sh(h), sh([h[3], h[5], h[3], h[5]]))], engine)
    with pytest.raises(MerkleTreeException, match="Cannot calculate Merkle root on empty hash list."):
        build_partial_trees([([], [])], engine)
    assert build_partial_trees([], engine) == []
    two = build_partial_trees([(sh([h[0], h[0]]), sh([h[0], h[0]]))], engine)[0]           # equal leaves, both listed
    assert two.flatten()[0] == [M.INCLUDED, M.INCLUDED, M.NODE]
    k, l, r, hs = two.flatten(5)
    assert PartialMerkleTree.unflatten([0] * 5 + k, [0] * 5 + l, [0] * 5 + r, [b""] * 5 + hs, 5, 8).flatten(5) == (k, l, r, hs)
