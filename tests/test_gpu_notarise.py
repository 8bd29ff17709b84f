"""cv_notarise_batch on the GPU (corda_amd/csrc/cv_api_notary.cpp, cv_k_notary.hip) against the composition of the
existing calls on the same inputs (tests/notarise_batches.py: Merkle ids -> verify over the ids -> missing signers ->
the restatement's gate -> cv_uniq_commit_batch on a second set loaded identically, keys = hashlib.sha256(leaf) ->
cv_ed25519_sign_keyed).  Every comparison is exact, array for array; signing is deterministic.

Shapes: ntx 1, 2 (the second transaction without leaves), 63, 64, 65, 130, 257 and 1100 (past the finalise scan's
workgroup of 1024), 1 to 3 signatures a transaction so that ranges straddle bitmap words, 0 to 4 leaves and 0 to 3
inputs, a set loaded with a few states.
"""
import numpy as np
import pytest

import notarise_batches as B
import notarise_cases as C
from corda_amd import native

pytestmark = pytest.mark.gpu

SHAPES = (1, 2, 63, 64, 65, 130, 257, 1100)
NAMES = ("outcome", "ids", "notary_sig", "first_bad", "req_missing", "state_conflict", "consumed_id", "consumed_index",
         "consumed_caller")


@pytest.fixture(scope="module")
def signer(engine):
    s = native.Signer(engine, B.NOTARY_SEED)
    yield s
    s.close()


_cache = {}


def expected(engine, corpus, signer, ntx, validating=True):
    """The batch and the comparator's results, computed once per shape and left unchanged."""
    key = (ntx, validating)
    if key not in _cache:
        if ntx not in _cache:
            _cache[ntx] = B.make_batch(engine, corpus, ntx)
        b = _cache[ntx]
        want, uniq = B.compose(engine, signer, b, validating)
        keys = np.concatenate([B.state_keys(b), b["resident"][0]])
        _cache[key] = (b, want, uniq, keys)
    return _cache[key]


def assert_same(got, want, what):
    for k in NAMES:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:8].tolist())


@pytest.mark.parametrize("ntx", SHAPES)
def test_equals_the_composition(engine, corpus, signer, ntx):
    b, want, ref_set, keys = expected(engine, corpus, signer, ntx)
    uniq = B.open_set(engine, b)
    got = B.call(engine, uniq, signer, b)
    assert_same(got, want, ntx)
    assert B.same_sets(uniq, ref_set, keys)
    out = got["outcome"]
    if ntx >= 63:
        assert set(out.tolist()) == set(range(9))          # every outcome code occurs
        assert b["expects_resident_conflict"] and all(out[t + 8] == C.CONFLICT for t in b["expects_resident_conflict"])
    # signatures: zero unless committed, and the notary's over the claimed id where committed
    acc = np.flatnonzero(out == C.SUCCESS)
    assert not got["notary_sig"][out != C.SUCCESS].any()
    if len(acc):
        pk = np.tile(np.frombuffer(signer.public_key, np.uint8), (len(acc), 1))
        bm, _ = engine.verify_batch(pk, got["notary_sig"][acc], b["claimed"].reshape(-1), (acc * 32).astype(np.uint64),
                                    np.full(len(acc), 32, np.uint32))
        assert native.bitmap_to_bools(bm, len(acc)).all()
    # first_bad names a signature of its own transaction, and only for the two signature outcomes
    named = got["first_bad"] != native.NS_NO_SIG
    assert (named <= np.isin(out, (C.TX_INVALID, C.BAD_KEY))).all()
    t = np.flatnonzero(named)
    assert ((got["first_bad"][t] >= b["tx_sig_begin"][t]) & (got["first_bad"][t] < b["tx_sig_begin"][t + 1])).all()
    uniq.close()


@pytest.mark.parametrize("ntx", (65, 257))
def test_not_validating(engine, corpus, signer, ntx):
    """validating = 0 with NULL signature and requirement arrays: the simple notary commits a transaction with bad
    signatures; only EMPTY, ID_MISMATCH, TIMESTAMP_INVALID, CONFLICT and SUCCESS occur."""
    b, want, ref_set, keys = expected(engine, corpus, signer, ntx, validating=False)
    uniq = B.open_set(engine, b)
    got = B.call(engine, uniq, signer, b, validating=False)
    assert_same(got, want, ntx)
    assert B.same_sets(uniq, ref_set, keys)
    assert set(got["outcome"].tolist()) == {C.SUCCESS, C.EMPTY, C.ID_MISMATCH, C.TIMESTAMP_INVALID, C.CONFLICT}
    bad = [t for t, k in enumerate(b["kind"]) if k in ("tx_invalid", "bad_key", "missing", "malformed", "prefilter")]
    assert bad and (got["outcome"][bad] == C.SUCCESS).all()      # their inputs are fresh: committed, as the reference does
    assert (got["first_bad"] == native.NS_NO_SIG).all()
    uniq.close()


@pytest.mark.parametrize("name,validating", (("no_inputs", False), ("no_signatures", True)))
def test_one_transaction_with_empty_pieces(engine, corpus, signer, name, validating):
    """ntx = 1 where whole groups of the call's arrays are empty: no input state under the simple notary (committed,
    nothing resident afterwards but what was loaded), and a validating call without any signature or requirement (the
    reference's SignedTransaction without signatures: TX_INVALID, no signature to name)."""
    b = B.edge_batch(engine, corpus, name)
    want, ref_set = B.compose(engine, signer, b, validating)
    uniq = B.open_set(engine, b)
    got = B.call(engine, uniq, signer, b, validating=validating)
    assert_same(got, want, name)
    assert B.same_sets(uniq, ref_set, np.concatenate([B.state_keys(b), b["resident"][0]]))
    assert got["outcome"].tolist() == [C.TX_INVALID if validating else C.SUCCESS]
    assert got["first_bad"].tolist() == [native.NS_NO_SIG] and got["notary_sig"].any() == (not validating)
    assert got["state_conflict"].size == (0 if name == "no_inputs" else int(b["tx_input_count"][0]))
    ref_set.close()
    uniq.close()


@pytest.mark.parametrize("rounds", (0, 1, 8))
def test_result_does_not_depend_on_max_rounds(engine, corpus, signer, rounds):
    """The chain at the end of the 130-transaction batch needs several rounds; 0 leaves everything to the serial tail."""
    b, want, ref_set, keys = expected(engine, corpus, signer, 130)
    uniq = B.open_set(engine, b)
    uniq.set_max_rounds(rounds)
    assert_same(B.call(engine, uniq, signer, b), want, rounds)
    assert B.same_sets(uniq, ref_set, keys)
    st = uniq.stats()
    assert st["rounds"] == rounds if rounds < 8 else st["rounds"] >= 2
    assert st["tail"] > 0 if rounds == 0 else True
    uniq.close()


def test_second_batch_sees_the_first(engine, corpus, signer):
    """The same batch again on the same set: every transaction that was committed now conflicts with itself."""
    b, want, _, _ = expected(engine, corpus, signer, 65)
    uniq = B.open_set(engine, b, capacity=400)
    first = B.call(engine, uniq, signer, b)
    again = B.call(engine, uniq, signer, b)
    has_inputs = b["tx_input_count"] > 0
    was = first["outcome"] == C.SUCCESS
    assert (again["outcome"][was & has_inputs] == C.CONFLICT).all()
    assert (again["outcome"][was & ~has_inputs] == C.SUCCESS).all()
    assert np.array_equal(again["outcome"][~was & (first["outcome"] != C.CONFLICT)], first["outcome"][~was & (first["outcome"] != C.CONFLICT)])
    sbeg = np.concatenate([[0], np.cumsum(b["tx_input_count"])])
    for t in np.flatnonzero(was & has_inputs)[:10]:
        s = slice(int(sbeg[t]), int(sbeg[t + 1]))
        assert again["state_conflict"][s].all() and (again["consumed_id"][s] == first["ids"][t]).all()
        assert (again["consumed_caller"][s] == b["caller"][t]).all()
    uniq.close()


def test_oom_and_bad_counts_touch_nothing(engine, corpus, signer):
    """CV_E_OOM (resident + nstates > capacity) leaves the set and every output buffer as they were; an input count
    above the transaction's leaf count is CV_E_ARGS, equally before anything is written."""
    b, _, _, keys = expected(engine, corpus, signer, 65)
    ns = int(b["tx_input_count"].sum())
    uniq = B.open_set(engine, b, capacity=len(b["resident"][0]) + ns - 1)
    before = (uniq.stats()["resident"], [a.copy() for a in uniq.lookup(keys)])
    rm = int(b["reqs"][6].size - 1)
    shapes = dict(outcome=(65,), ids=(65, 32), notary_sig=(65, 64), first_bad=(65,), req_missing=(rm,), state_conflict=(ns,),
                  consumed_id=(ns, 32), consumed_index=(ns,), consumed_caller=(ns,))
    u32 = ("first_bad", "consumed_index", "consumed_caller")
    for tamper, code in ((False, -4), (True, -3)):
        out = {k: np.full(s, 0xABABABAB if k in u32 else 0xAB, np.uint32 if k in u32 else np.uint8) for k, s in shapes.items()}
        bb = dict(b)
        if tamper:
            bb["tx_input_count"] = b["tx_input_count"].copy()
            bb["tx_input_count"][3] = 5
        with pytest.raises(native.CvError) as e:
            B.call(engine, uniq, signer, bb, out=out)
        assert e.value.code == code
        assert all((a.view(np.uint8) == 0xAB).all() for a in out.values())
        assert uniq.stats()["resident"] == before[0]
        assert all(np.array_equal(x, y) for x, y in zip(uniq.lookup(keys), before[1]))
    uniq.reserve(len(b["resident"][0]) + ns)
    assert (B.call(engine, uniq, signer, b)["outcome"] == C.SUCCESS).any()
    uniq.close()
