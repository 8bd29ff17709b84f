"""cv_resolve_batch on the GPU against the restatement of ResolveTransactionsFlow.call (tests/resolve_cases.py): every
case at every batch size through Engine.resolve_batch, the per-transaction verdicts against the three component calls
on the same batch, the Python mirror's fused path against its composition, a seed under which a probe wraps, and two
seeds with one result.
"""
import hashlib

import numpy as np
import pytest

import resolve_cases as C
from corda_amd import native, resolve
from corda_amd.crypto import DigitalSignature, KeyPair
from corda_amd.transactions import MerkleTree, SecureHash, SignedTransaction, WireTransaction

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", C.SIZES)
def test_every_case_equals_the_reference(engine, corpus, n):
    """Every output equals resolve_ref over what cv_merkle_tx_ids_bounded + cv_ed25519_verify_batch +
    cv_missing_signers give on the same batch; ids and req_missing equal theirs; and the faults planted in the data are
    the ones the case names (the outcome of the plain transactions)."""
    ran = 0
    for name, build in C.CASES.items():
        specs = build(n)
        if specs is None:
            continue
        b = C.real(engine, corpus, specs)
        txs, ids, req_missing = C.components(engine, b)
        want = C.resolve_ref(txs)
        got = engine.resolve_batch(**b, seed=1 + ran)
        C.same(got, want, (name, n))
        assert np.array_equal(got["ids"], ids) and np.array_equal(got["req_missing"], req_missing), (name, n)
        assert np.array_equal(want["outcome"], C.resolve_ref(C.concrete(specs))["outcome"]), (name, n)
        ran += 1
    assert ran >= 5                                    # chain, reversed chain, outside only, no inputs, self-reference


def _nothing_to_check(engine, corpus):
    """One transaction with leaves and nothing else: N = nreq = nnodes = nchild = ninputs = 0."""
    b = C.real(engine, corpus, [C.spec()])
    none, u32 = np.zeros((0, 32), np.uint8), lambda *a: np.array(a, np.uint32)
    b["sigs"] = (none, np.zeros((0, 64), np.uint8), u32(0, 0), None)
    b["reqs"] = (np.zeros(0, np.uint8), none, np.zeros(0, np.int32), u32(0), u32(), np.zeros(0, np.int32), u32(0), u32(0, 0),
                 none)
    return b


def _one_signature_each(engine, corpus):
    """65 transactions with one signature each, the one their requirement names: the verdict bitmap crosses a word."""
    b = C.real(engine, corpus, C.chain(65))
    pk, sig, _, _ = b["sigs"]
    b["sigs"] = (pk[1::2].copy(), sig[1::2].copy(), np.arange(66, dtype=np.uint32), None)
    b["reqs"] = b["reqs"][:8] + (pk[1::2].copy(),)
    return b


@pytest.mark.parametrize("build, outcome", ((_nothing_to_check, native.CV_RS_TX_INVALID),
                                            (_one_signature_each, native.CV_RS_OK)))
def test_empty_pieces_equal_the_reference(engine, corpus, build, outcome):
    """Pieces of the call's one buffer at zero bytes, and one signature a transaction (a transaction without leaves is
    C.CASES["empty_mid_chain"], one without inputs "no_inputs", both in test_every_case_equals_the_reference).  A
    transaction without signatures is invalid (the reference's "no_signatures" case); the others pass."""
    b = build(engine, corpus)
    txs, ids, req_missing = C.components(engine, b)
    got = engine.resolve_batch(**b, seed=3)
    C.same(got, C.resolve_ref(txs), build.__name__)
    assert np.array_equal(got["ids"], ids) and np.array_equal(got["req_missing"], req_missing)
    assert (got["outcome"] == outcome).all()


def test_optional_outputs_and_fresh_seed(engine, corpus):
    """seed 0 draws one; the optional outputs may be left out."""
    b = C.real(engine, corpus, C.CASES["diamond"](65))
    want = C.resolve_ref(C.components(engine, b)[0])
    got = engine.resolve_batch(**b, out={"first_bad": None, "req_missing": None, "ids": None})
    assert got["first_bad"] is None and got["req_missing"] is None and got["ids"] is None
    C.same(got, {k: v for k, v in want.items() if k != "first_bad"})


def test_a_probe_wraps_under_the_chosen_seed(engine, corpus):
    """resolve_cases.WRAP_SEED was chosen with the CPU harness (tests/test_resolve_cpu.py checks it there)."""
    b = C.real(engine, corpus, C.CASES["chain"](65))
    got = engine.resolve_batch(**b, seed=C.WRAP_SEED)
    C.same(got, C.resolve_ref(C.components(engine, b)[0]))
    assert got["graph"][8] > 0 and got["graph"][7] >= 2


def test_two_seeds_one_result(engine, corpus):
    b = C.real(engine, corpus, C.CASES["fan_in"](1025))
    a, c = engine.resolve_batch(**b, seed=7), engine.resolve_batch(**b, seed=0x9e3779b97f4a7c15)
    for k in a:
        assert np.array_equal(a[k][:C.G_COMPARED] if k == "graph" else a[k], c[k][:C.G_COMPARED] if k == "graph" else c[k]), k


# ---------------------------------------------------------------- the mirror
def _host_id(wtx) -> SecureHash:
    return MerkleTree.get_merkle_tree([SecureHash(hashlib.sha256(b).digest()) for b in wtx.leaves]).hash


@pytest.fixture(scope="module")
def keys(engine):
    ks = [KeyPair(hashlib.sha256(b"resolve key %d" % k).digest(), engine) for k in range(3)]
    yield ks
    for k in ks:
        k.close()


def _graph(keys, shape, n=9):
    """n transactions, built oldest first (an input names its dependency's id), signed by keys 0 and 1; returned in
    download order, the newest first.  shape: "chain", or "diamond" (the newest spends two that spend one)."""
    outside = SecureHash(hashlib.sha256(b"outside").digest())
    wtxs = []
    for t in range(n):
        if t == 0:
            refs = [resolve.StateRef(outside, 0)]
        elif shape == "diamond" and t == n - 1:
            refs = [resolve.StateRef(wtxs[t - 1]._id, 0), resolve.StateRef(wtxs[t - 2]._id, 1)]
        elif shape == "diamond" and t == n - 2:
            refs = [resolve.StateRef(wtxs[t - 2]._id, 1)]
        else:
            refs = [resolve.StateRef(wtxs[t - 1]._id, 0)]
        w = WireTransaction(inputs=[r.blob for r in refs], outputs=[b"out %d a" % t, b"out %d b" % t],
                            commands=[b"cmd %d" % t], must_sign=[keys[0].public.composite, keys[1].public.composite])
        w._id = _host_id(w)
        wtxs.append(w)
    sigs = [k.sign_many([w._id.bytes for w in wtxs]) for k in keys[:2]]
    return [SignedTransaction(w, [sigs[0][t], sigs[1][t]], w._id) for t, w in enumerate(wtxs)][::-1]


def _same_result(a, b):
    assert [s.id for s in a[0]] == [s.id for s in b[0]] and a[1] == b[1]
    assert type(a[2]) is type(b[2]) and str(a[2]) == str(b[2])


def test_mirror_fused_equals_composition(engine, keys):
    """resolve_transactions(fused=True) against fused=False, exception for exception, over a clean chain and diamond,
    a bad signature, a missing signer, an id mismatch, a duplicate and an out-of-range index."""
    runs = []
    for shape in ("chain", "diamond"):
        stxs = _graph(keys, shape)
        runs.append((shape, stxs, type(None)))
    stxs = _graph(keys, "chain")
    s = stxs[4]
    s.sigs[1] = DigitalSignature.WithKey(s.sigs[1].by, bytes([s.sigs[1].bits[0] ^ 1]) + s.sigs[1].bits[1:])
    runs.append(("bad signature", stxs, resolve.SignatureException))
    stxs = _graph(keys, "chain")
    stxs[3]._wtx.must_sign.append(keys[2].public.composite)
    runs.append(("missing signer", stxs, resolve.SignatureException))
    stxs = _graph(keys, "chain")
    stxs[5].id = SecureHash(hashlib.sha256(b"not it").digest())
    runs.append(("id mismatch", stxs, resolve.IllegalStateException))
    stxs = _graph(keys, "chain")
    runs.append(("duplicate", stxs + [stxs[2]], resolve.IllegalStateException))
    stxs = _graph(keys, "chain")
    stxs[6]._wtx.outputs = []              # the outputs are not among the leaves the id was hashed over ...
    stxs[6]._wtx._id = None
    runs.append(("re-hashed", stxs, resolve.IllegalStateException))      # ... so this is an id mismatch too
    for what, stxs, exc in runs:
        fused = resolve.resolve_transactions(stxs, engine, fused=True)
        composed = resolve.resolve_transactions(stxs, engine, fused=False)
        _same_result(fused, composed)
        assert isinstance(fused[2], exc), what
        if exc is type(None):
            assert fused[1] == len(stxs) and [s.id for s in fused[0]] == [s.id for s in stxs[::-1]]
    # an index past the dependency's outputs: the newest transaction names output 2 of a dependency with two
    outside = _graph(keys, "chain", 3)[::-1]
    w = WireTransaction(inputs=[resolve.StateRef(outside[2].id, 2).blob], outputs=[b"o"], commands=[b"c"],
                        must_sign=[keys[0].public.composite])
    w._id = _host_id(w)
    top = SignedTransaction(w, keys[0].sign_many([w._id.bytes]), w._id)
    stxs = [top] + outside[::-1]
    fused = resolve.resolve_transactions(stxs, engine, fused=True)
    _same_result(fused, resolve.resolve_transactions(stxs, engine, fused=False))
    assert isinstance(fused[2], IndexError) and fused[1] == 3 and fused[0][3] is top
