"""cv_filtered_verify and cv_tearoff_sign_batch on the GPU (corda_amd/csrc/cv_api_tearoff.cpp, cv_k_tearoff.hip)
against the calls they fuse, result for result, and against the restatement of the reference (tests/tearoff_cases.py
over oracle/merkle_ref.py): the verify against cv_partial_merkle_verify fed hashlib's check hashes, the signing call
against cv_filtered_verify + the gate in Python + cv_ed25519_sign_keyed over the accepted roots.
"""
import hashlib
import os

import numpy as np
import pytest

import ed25519_ref
import merkle_ref as M
import tearoff_cases as C
from corda_amd import native

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
SEED2 = bytes(range(1, 33))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "partial_merkle_cases.npz")


@pytest.fixture(scope="module")
def signer(engine):
    s = native.Signer(engine, SEED)
    yield s
    s.close()


def verify_args(f):
    return (f["arena"], f["leaf_off"], f["leaf_len"], f["txb"], f["kind"], f["left"], f["right"], f["node_hash"],
            f["tree_begin"], f["root"])


def two_step(engine, f):
    """The path cv_filtered_verify replaces: the filtered hashes made on the host, then cv_partial_merkle_verify —
    with FilteredTransaction.verify's empty check, which that path leaves to the caller."""
    a = f["arena"].tobytes()
    check = [hashlib.sha256(a[int(o):int(o) + int(n)]).digest() for o, n in zip(f["leaf_off"], f["leaf_len"])]
    rows = np.frombuffer(b"".join(check), np.uint8).reshape(-1, 32) if check else np.zeros((0, 32), np.uint8)
    v, st = engine.partial_merkle_verify(f["kind"], f["left"], f["right"], f["node_hash"], f["tree_begin"], f["root"], rows,
                                         f["txb"])
    empty = f["txb"][1:] == f["txb"][:-1]
    return np.where(empty, 0, v).astype(np.uint8), np.where(empty, C.PMT_NO_INCLUDED, st).astype(np.uint8)


def verify_cases():
    """Trees over 1, 2, 3, 5, 6, 8 and 9 leaves (odd duplication at several levels) with the first leaf, the last leaf
    (the duplicated one) and all leaves kept; two equal blobs; every tampering; no filtered leaves."""
    txs, lengths = [], set()
    for n in (1, 2, 3, 5, 6, 8, 9):
        w = C.wire(n, 11 * n)
        lengths |= {len(lf["blob"]) for lf in w}
        for keep in ([0], [n - 1], list(range(n))):
            txs.append(C.tearoff(w, keep))
    assert lengths >= set(C.BLOB_LENGTHS)
    n_honest = len(txs)
    twin = C.wire(5, 77)
    twin[3] = dict(twin[3], blob=twin[1]["blob"])                  # the multiset case: both must be kept and checked
    txs.append(C.tearoff(twin, [1, 3]))
    txs.append(C.tearoff(twin, [0, 1, 3]))
    n_ok = len(txs)
    base = C.tearoff(C.wire(6, 5), [1, 4])
    lv = base["leaves"]
    txs.append(C.tampered(base, leaves=[dict(lv[0], blob=C.flip(lv[0]["blob"], 3)), lv[1]]))     # a flipped blob byte
    txs.append(C.tampered(base, root=C.flip(base["root"], 31)))                                  # a wrong root
    txs.append(C.tampered(base, leaves=lv + [C.leaf(b"one too many")]))
    txs.append(C.tampered(base, leaves=lv[:1]))                                                  # one too few
    txs.append(C.tampered(C.tearoff(twin, [1, 3]), leaves=[twin[1]]))                            # ... of two equal blobs
    txs.append(C.tearoff(C.wire(4, 9), []))                                                      # no filtered leaves
    txs.append(C.tampered(base, leaves=[]))
    return txs, n_honest, n_ok


VERIFY_CASES, N_HONEST, N_OK = verify_cases()


def test_filtered_verify_equals_the_two_step_path_and_the_oracle(engine):
    f = C.flatten(VERIFY_CASES)
    want = C.expected(VERIFY_CASES)
    assert want["verdict"][:N_OK].all() and not want["verdict"][N_OK:].any()
    assert (want["status"][-2:] == C.PMT_NO_INCLUDED).all() and not want["status"][:-2].any()
    v, st = engine.filtered_verify(*verify_args(f))
    v2, st2 = two_step(engine, f)
    assert np.array_equal(v, v2) and np.array_equal(st, st2)
    assert np.array_equal(v, want["verdict"]) and np.array_equal(st, want["status"])
    # the same through the object layer, one batch without the throwing items
    from corda_amd.transactions import (FilteredLeaves, FilteredTransaction, PartialMerkleTree, SecureHash,
                                        verify_filtered_batch_fused)
    items = []
    for tx in VERIFY_CASES[:-2]:
        k, l, r, h = tx["nodes"]
        pmt = PartialMerkleTree.unflatten(k, l, r, h, 0, len(k))
        items.append((FilteredTransaction(FilteredLeaves(commands=[lf["blob"] for lf in tx["leaves"]]), pmt),
                      SecureHash(tx["root"])))
    assert verify_filtered_batch_fused(items, engine) == [bool(x) for x in want["verdict"][:-2]]


def test_filtered_verify_malformed_encodings(engine):
    """The malformed encodings of the golden fixture: status CV_PMT_MALFORMED and verdict 0 whatever the leaves are,
    as cv_partial_merkle_verify says over the same leaves' hashes — unless there is no leaf, which wins."""
    c = dict(np.load(GOLDEN))
    bad = np.nonzero(c["status"] == C.PMT_MALFORMED)[0]
    assert bad.size
    kind, left, right, hashes, tb, roots, txb, blobs = [], [], [], [], [0], [], [0], []
    for j, t in enumerate(bad):
        b, e = int(c["tree_begin"][t]), int(c["tree_begin"][t + 1])
        base = len(kind)
        kind += c["kind"][b:e].tolist()
        # children stay where they point inside the tree: the same offsets from the tree's new first node
        left += [(int(x) - b + base) & 0xFFFFFFFF for x in c["left"][b:e]]
        right += [(int(x) - b + base) & 0xFFFFFFFF for x in c["right"][b:e]]
        hashes += [c["leaf_hash"][k].tobytes() for k in range(b, e)]
        tb.append(len(kind))
        roots.append(c["root"][t].tobytes())
        blobs += [b"leaf %d.%d" % (t, i) for i in range(j % 3)]           # 0, 1 or 2 filtered leaves
        txb.append(len(blobs))
    lens = np.array([len(x) for x in blobs], np.uint32)
    f = {"arena": np.frombuffer(b"".join(blobs) + bytes(16), np.uint8).copy(), "leaf_len": lens,
         "leaf_off": (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64), "txb": np.array(txb, np.uint32),
         "kind": np.array(kind, np.uint8), "left": np.array(left, np.uint32), "right": np.array(right, np.uint32),
         "node_hash": np.frombuffer(b"".join(hashes), np.uint8).reshape(-1, 32) if hashes else np.zeros((0, 32), np.uint8),
         "tree_begin": np.array(tb, np.uint32), "root": np.frombuffer(b"".join(roots), np.uint8).reshape(-1, 32)}
    v, st = engine.filtered_verify(*verify_args(f))
    v2, st2 = two_step(engine, f)
    assert np.array_equal(v, v2) and np.array_equal(st, st2)
    empty = f["txb"][1:] == f["txb"][:-1]
    assert not v.any() and np.array_equal(st, np.where(empty, C.PMT_NO_INCLUDED, C.PMT_MALFORMED))


def test_round_trip_with_filtered_build(engine):
    """cv_filtered_build's output into cv_filtered_verify with the kept blobs: every verdict 1, ids = the roots."""
    rng = np.random.default_rng(21)
    wires = [C.wire(n, 100 + n) for n in (1, 2, 3, 5, 6, 8, 9, 17)]
    all_blobs = [lf["blob"] for w in wires for lf in w]
    keep = rng.integers(0, 2, len(all_blobs)).astype(np.uint8)
    begin = np.cumsum([0] + [len(w) for w in wires]).astype(np.uint32)
    for t in range(len(wires)):
        keep[begin[t]] = 1                                           # at least one kept leaf a transaction
    lens = np.array([len(b) for b in all_blobs], np.uint32)
    offs = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
    arena = np.frombuffer(b"".join(all_blobs) + bytes(16), np.uint8)
    kind, left, right, hashes, tb, ids, st = engine.filtered_build(arena, offs, lens, begin, keep)
    assert not st.any()
    kept = np.nonzero(keep)[0]
    kb = np.searchsorted(kept, begin).astype(np.uint32)              # the kept leaves of every transaction
    v, vst = engine.filtered_verify(arena, offs[kept], lens[kept], kb, kind, left, right, hashes, tb, ids)
    assert v.all() and not vst.any()
    for t, w in enumerate(wires):
        assert ids[t].tobytes() == M.get_merkle_tree([M.sha256(lf["blob"]) for lf in w]).hash


def compose(engine, signer, f, with_pre=True):
    """What a binding did before the fused call: cv_filtered_verify, the gate in Python, cv_ed25519_sign_keyed over the
    accepted roots, the signatures scattered into zeros."""
    v, st = engine.filtered_verify(*verify_args(f))
    out, fb = C.python_gate(f["txb"], v, st, f["leaf_pre"] if with_pre else None)
    acc = np.nonzero(out == C.SUCCESS)[0]
    sig = np.zeros((f["ntx"], 64), np.uint8)
    if acc.size:
        sig[acc] = signer.sign(f["root"].reshape(-1), 32 * acc.astype(np.uint64), np.full(acc.size, 32, np.uint32))
    return out, fb, sig


@pytest.mark.parametrize("ntx", [1, 64, 65, 1025])
def test_fused_call_equals_the_composition(engine, signer, ntx):
    txs = C.service_batch(ntx, seed=1000 * ntx)
    f = C.flatten(txs)
    want = C.expected(txs)
    if ntx >= 64:
        assert set(want["outcome"].tolist()) == set(range(7))
        assert abs(int((want["outcome"] != 0).sum()) - ntx // 8) <= 1
    out, fb, sig = engine.tearoff_sign_batch(signer, *verify_args(f), f["leaf_pre"])
    c_out, c_fb, c_sig = compose(engine, signer, f)
    assert np.array_equal(out, c_out) and np.array_equal(fb, c_fb) and np.array_equal(sig, c_sig)
    assert np.array_equal(out, want["outcome"]) and np.array_equal(fb, want["first_bad"])
    acc = want["accepted"]
    assert not sig[out != C.SUCCESS].any()
    for t in acc[:16]:
        assert sig[t].tobytes() == ed25519_ref.sign(SEED, f["root"][t].tobytes())
    pk = np.tile(np.frombuffer(signer.public_key, np.uint8), (acc.size, 1))
    bitmap, _ = engine.verify_batch(pk, sig[acc], f["root"].reshape(-1), 32 * acc.astype(np.uint64),
                                    np.full(acc.size, 32, np.uint32))
    bits = np.unpackbits(bitmap.view(np.uint8), bitorder="little")[:acc.size]
    assert bits.all()


@pytest.mark.parametrize("name", list(C.edge_batches()))
def test_edge_batches_equal_the_composition_and_the_oracle(engine, signer, name):
    """ntx = 1 with no leaf and no node, the same between two ordinary tear-offs, and three tear-offs none of which is
    accepted (nothing is signed): the verify against the two-step path, the signing call against the composition,
    both against the restatement; then with leaf_pre NULL."""
    txs = C.edge_batches()[name]
    f, want = C.flatten(txs), C.expected(txs)
    if name == "three_refused":
        assert not want["accepted"].size
    v, st = engine.filtered_verify(*verify_args(f))
    v2, st2 = two_step(engine, f)
    assert np.array_equal(v, v2) and np.array_equal(st, st2)
    assert np.array_equal(v, want["verdict"]) and np.array_equal(st, want["status"])
    out, fb, sig = engine.tearoff_sign_batch(signer, *verify_args(f), f["leaf_pre"])
    c_out, c_fb, c_sig = compose(engine, signer, f)
    assert np.array_equal(out, c_out) and np.array_equal(fb, c_fb) and np.array_equal(sig, c_sig)
    assert np.array_equal(out, want["outcome"]) and np.array_equal(fb, want["first_bad"])
    assert not sig[out != C.SUCCESS].any()
    for t in want["accepted"]:
        assert sig[t].tobytes() == ed25519_ref.sign(SEED, f["root"][t].tobytes())
    out, fb, sig = engine.tearoff_sign_batch(signer, *verify_args(f), None)
    c_out, c_fb, c_sig = compose(engine, signer, f, with_pre=False)
    assert np.array_equal(out, c_out) and np.array_equal(fb, c_fb) and np.array_equal(sig, c_sig)


def test_null_leaf_pre_and_null_first_bad(engine, signer):
    txs = C.service_batch(65, seed=7)
    f = C.flatten(txs)
    out, fb, sig = engine.tearoff_sign_batch(signer, *verify_args(f), None)
    c_out, c_fb, c_sig = compose(engine, signer, f, with_pre=False)
    assert np.array_equal(out, c_out) and np.array_equal(fb, c_fb) and np.array_equal(sig, c_sig)
    assert (fb == C.NO_LEAF).all() and set(out.tolist()) == {C.SUCCESS, C.NO_LEAVES, C.MALFORMED, C.VERIFY_FAILED}
    o2, s2 = np.zeros(65, np.uint8), np.zeros((65, 64), np.uint8)
    engine.tearoff_sign_batch(signer, *verify_args(f), None, out=(o2, None, s2))
    assert np.array_equal(o2, out) and np.array_equal(s2, sig)


def test_a_second_signer_gives_other_signatures(engine, signer):
    txs = C.service_batch(64, seed=3)
    f = C.flatten(txs)
    out1, _, sig1 = engine.tearoff_sign_batch(signer, *verify_args(f), f["leaf_pre"])
    with native.Signer(engine, SEED2) as other:
        out2, _, sig2 = engine.tearoff_sign_batch(other, *verify_args(f), f["leaf_pre"])
        pk2 = other.public_key
    acc = np.nonzero(out1 == C.SUCCESS)[0]
    assert np.array_equal(out1, out2) and acc.size
    assert not (sig1[acc] == sig2[acc]).all(1).any() and not sig2[out2 != C.SUCCESS].any()
    assert pk2 != signer.public_key
    for t in acc[:4]:
        assert sig2[t].tobytes() == ed25519_ref.sign(SEED2, f["root"][t].tobytes())


def test_every_device_slot_of_a_context_signs(engine, signer):
    """A context of two device slots: successive calls land on different slots, each with the signer's record."""
    txs = C.service_batch(16, seed=11)
    f = C.flatten(txs)
    want = engine.tearoff_sign_batch(signer, *verify_args(f), f["leaf_pre"])
    with native.Engine(1, virtual_devices=2) as e2, native.Signer(e2, SEED) as s2:
        for _ in range(3):
            got = e2.tearoff_sign_batch(s2, *verify_args(f), f["leaf_pre"])
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
            v, st = e2.filtered_verify(*verify_args(f))
            assert np.array_equal(v, C.expected(txs)["verdict"])


def test_the_object_layer_returns_the_references_exceptions(engine, signer):
    """corda_amd.tearoff.TearOffOracle.sign_batch: per item the signature or what Oracle.sign would throw."""
    from corda_amd.tearoff import TearOffOracle, UnknownFix
    from corda_amd.transactions import (FilteredLeaves, FilteredTransaction, MerkleTreeException, PartialMerkleTree,
                                        SecureHash)
    from corda_amd.crypto import IllegalArgumentException
    txs = C.service_batch(64, seed=3)
    by_blob = {lf["blob"]: lf for tx in txs for lf in tx["leaves"]}
    items = []
    for tx in txs:
        k, l, r, h = tx["nodes"]
        groups = {g: [lf["blob"] for lf in tx["leaves"] if lf["group"] == g] for g in C.GROUPS}
        pmt = PartialMerkleTree.unflatten(k, l, r, h, 0, len(k)) if tx["tree"] is not None or k[0] <= 2 else None
        if pmt is None:
            continue                      # the object layer cannot hold nodes of an unknown kind
        items.append((tx, FilteredTransaction(FilteredLeaves(**groups), pmt), SecureHash(tx["root"])))
    oracle = TearOffOracle(signer, lambda group, b: C.classify(dict(by_blob[b], group=group)))
    res = oracle.sign_batch([(ftx, root) for _, ftx, root in items])
    want = C.expected([tx for tx, _, _ in items])["outcome"]
    kinds = {C.NO_LEAVES: MerkleTreeException, C.VERIFY_FAILED: MerkleTreeException,
             C.NOT_COMMANDS: IllegalArgumentException, C.WRONG_COMMAND: IllegalArgumentException, C.UNKNOWN: UnknownFix}
    assert set(want.tolist()) >= set(kinds)
    assert res[0] == ed25519_ref.sign(SEED, items[0][2].bytes)
    for (tx, _, root), r, o in zip(items, res, want):
        if o == C.SUCCESS:
            assert isinstance(r, bytes) and len(r) == 64 and any(r)
        else:
            assert type(r) is kinds[int(o)]
            if o == C.UNKNOWN:
                assert r.leaf == 0 and r.leaf_bytes == tx["leaves"][0]["blob"]


def test_refused_calls_write_nothing(engine, signer):
    """CV_E_ARGS and CV_E_TOO_LARGE come before any device work and any output."""
    lib, P = native.load(), native._p
    f = C.flatten(C.service_batch(8, seed=5))
    n = f["ntx"]
    poison = lambda m, dt=np.uint8: np.full(m, 0xA5 if dt == np.uint8 else 0xA5A5A5A5, dt)      # noqa: E731

    def call(ntx=n, txb=f["txb"], pre=f["leaf_pre"], arena_bytes=f["arena_bytes"], verify=True):
        out = (poison(n), poison(n, np.uint32), poison(64 * n), poison(n), poison(n))
        nodes = [P(f[k]) for k in ("kind", "left", "right", "node_hash")]
        rc1 = lib.cv_tearoff_sign_batch(engine._h, signer._h, ntx, P(f["arena"]), arena_bytes, P(f["leaf_off"]),
                                        P(f["leaf_len"]), P(txb), len(f["kind"]), *nodes, P(f["tree_begin"]), P(f["root"]),
                                        P(pre), P(out[0]), P(out[1]), P(out[2]))
        rc2 = lib.cv_filtered_verify(engine._h, ntx, P(f["arena"]), arena_bytes, P(f["leaf_off"]), P(f["leaf_len"]), P(txb),
                                     len(f["kind"]), *nodes, P(f["tree_begin"]), P(f["root"]), P(out[3]),
                                     P(out[4])) if verify else None
        assert all((a == poison(1, a.dtype)[0]).all() for a in out)
        return rc1, rc2
    bad_pre = f["leaf_pre"].copy()
    bad_pre[-1] = 4
    assert call(pre=bad_pre, verify=False)[0] == -3            # (the verify takes no leaf_pre)
    bad_txb = f["txb"].copy()
    bad_txb[0] = 1
    assert call(txb=bad_txb) == (-3, -3)
    assert call(arena_bytes=f["arena_bytes"] - 1) == (-3, -3)
    assert call(ntx=0xffffffff) == (-5, -5)
    assert call(ntx=0) == (0, 0)
    # a signer of another context is refused too
    with native.Engine(1) as e2, native.Signer(e2, SEED) as s2:
        out = (poison(n), poison(64 * n))
        nodes = [P(f[k]) for k in ("kind", "left", "right", "node_hash")]
        assert lib.cv_tearoff_sign_batch(engine._h, s2._h, n, P(f["arena"]), f["arena_bytes"], P(f["leaf_off"]),
                                         P(f["leaf_len"]), P(f["txb"]), len(f["kind"]), *nodes, P(f["tree_begin"]),
                                         P(f["root"]), P(f["leaf_pre"]), P(out[0]), None, P(out[1])) == -3
        assert (out[0] == 0xA5).all() and (out[1] == 0xA5).all()
