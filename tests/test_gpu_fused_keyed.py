"""CV_OPT_FUSED_KEYED on the GPU: cv_resolve_batch and cv_notarise_batch with the keyed verify route never taken (0) and
always taken (2) — every case of tests/resolve_cases.py at its sizes and every group of tests/notarise_cases.py (as
real batches, tests/notarise_real.py): every output equal array for array between the two settings and equal to the
reference over the component calls, as tests/test_gpu_resolve.py and tests/test_gpu_notarise.py compare.  That the
keyed route ran is read off cv_key_cache_stats on an engine of this module's own, whose key pool nothing else uses:
misses rise by the distinct keys at the first call under 2, only hits at the second, nothing under 0; auto (1) takes
the route for a chain of 5,000 and not for 64 signatures; a batch with more distinct keys than the pool's capacity
stays unkeyed and leaves the pool alone.  A repeated bad key as the first failing signature gives BAD_KEY and the same
first_bad under both.
"""
import numpy as np
import pytest

import keydedupe_cases as K
import notarise_batches as B
import notarise_cases as NC
import notarise_real
import resolve_cases as C
from guarded import Options
from corda_amd import native

pytestmark = pytest.mark.gpu

NOTARY_NAMES = ("outcome", "ids", "notary_sig", "first_bad", "req_missing", "state_conflict", "consumed_id",
                "consumed_index", "consumed_caller")


def equal(a, b, what):
    """Array for array; of a resolve call's graph the words resolve_cases.same compares — the other two are the join
    table's longest probe and its wraps, which depend on which lane claimed a slot first."""
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = (a[k][:C.G_COMPARED], b[k][:C.G_COMPARED]) if k == "graph" else (a[k], b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), (what, k)


def resolve_both(engine, b, seed):
    """The call under 0 and under 2 with one seed."""
    with Options(engine, fused_keyed=0):
        plain = engine.resolve_batch(**b, seed=seed)
    with Options(engine, fused_keyed=2):
        keyed = engine.resolve_batch(**b, seed=seed)
    return plain, keyed


@pytest.mark.parametrize("n", C.SIZES)
def test_resolve_cases_under_0_and_2(engine, corpus, n):
    ran = 0
    for name, build in C.CASES.items():
        specs = build(n)
        if specs is None:
            continue
        b = C.real(engine, corpus, specs)
        txs, ids, req_missing = C.components(engine, b)
        want = C.resolve_ref(txs)
        plain, keyed = resolve_both(engine, b, 1 + ran)
        equal(plain, keyed, (name, n))
        C.same(keyed, want, (name, n))
        assert np.array_equal(keyed["ids"], ids) and np.array_equal(keyed["req_missing"], req_missing), (name, n)
        ran += 1
    assert ran >= 5


@pytest.fixture(scope="module")
def signer(engine):
    s = native.Signer(engine, B.NOTARY_SEED)
    yield s
    s.close()


def notarise_under(engine, signer, b, mode):
    """A fresh set per setting, so the commits match."""
    uniq = B.open_set(engine, b)
    with Options(engine, fused_keyed=mode):
        got = B.call(engine, uniq, signer, b)
    return got, uniq


@pytest.mark.parametrize("name", list(NC.CASES))
def test_notary_groups_under_0_and_2(engine, corpus, signer, name):
    txs, resident = NC.CASES[name]()
    b, plain = notarise_real.realise(engine, corpus, txs, resident)
    want, ref_set = B.compose(engine, signer, b)
    keys = np.concatenate([B.state_keys(b), b["resident"][0]])
    got = {}
    for mode in (0, 2):
        got[mode], uniq = notarise_under(engine, signer, b, mode)
        for k in NOTARY_NAMES:
            assert got[mode][k].shape == want[k].shape and np.array_equal(got[mode][k], want[k]), (name, mode, k)
        assert B.same_sets(uniq, ref_set, keys), (name, mode)
        uniq.close()
    equal(got[0], got[2], name)
    ref_set.close()
    # the batch plants what the group names: the outcomes are the restatement's over the plain cases
    assert np.array_equal(want["outcome"], NC.notarise(plain, True, resident)["outcome"]), name


# ---------------------------------------------------------------- which route ran
@pytest.fixture(scope="module")
def own():
    """An engine whose key pool only this module's calls use, kept small (66 KB of tables a key)."""
    e = native.Engine(1)
    e.key_cache_reserve(64)
    yield e
    e.close()


def moved(engine, before):
    st = engine.key_cache_stats(0)
    return st["hits"] - before["hits"], st["misses"] - before["misses"]


def test_stats_show_the_route(own, corpus):
    """chain(64): 128 signatures under the four keys of resolve_cases._signed."""
    b = C.real(own, corpus, C.chain(64))
    nkeys = K.reference(b["sigs"][0])[2]
    assert nkeys == 4
    st = own.key_cache_stats(0)
    with Options(own, fused_keyed=0):
        first = own.resolve_batch(**b, seed=5)
    assert moved(own, st) == (0, 0)
    with Options(own, fused_keyed=2):
        second = own.resolve_batch(**b, seed=5)
        assert moved(own, st) == (0, nkeys)                 # one lookup a distinct key, all new
        third = own.resolve_batch(**b, seed=5)
        assert moved(own, st) == (nkeys, nkeys)             # the same keys again: only hits
    equal(first, second, "0 against 2")
    equal(second, third, "2 again")
    with Options(own, fused_keyed=1):
        own.resolve_batch(**b, seed=5)
    assert moved(own, st) == (nkeys, nkeys)                 # auto: 128 signatures stay below the tri-chain size


def test_notary_stats_show_the_route(corpus):
    """The notary's call takes the device's key pool under its set's lock: the lookups count as the resolve call's.  An
    engine of the test's own, so every key of the batch is new to its pool."""
    e = native.Engine(1)
    e.key_cache_reserve(64)
    signer = native.Signer(e, B.NOTARY_SEED)
    sets = []
    try:
        b = B.make_batch(e, corpus, 65)
        nkeys = K.reference(b["pk"])[2]
        st = e.key_cache_stats(0)
        got0, u = notarise_under(e, signer, b, 0)
        sets.append(u)
        assert moved(e, st) == (0, 0)
        got2, u = notarise_under(e, signer, b, 2)
        sets.append(u)
        assert moved(e, st) == (0, nkeys)                   # misses rise by the distinct keys
        equal(got0, got2, "notary 0 against 2")
        got2b, u = notarise_under(e, signer, b, 2)
        sets.append(u)
        assert moved(e, st) == (nkeys, nkeys)               # the same keys again: only hits
        equal(got2, got2b, "notary 2 again")
    finally:
        for u in sets:
            u.close()
        signer.close()
        e.close()


def test_auto_takes_a_long_chain_and_not_64_signatures(own, corpus):
    """Auto (1): a chain of 5,000 transactions — 10,000 signatures, four keys — takes the keyed route; 64 signatures,
    whatever their keys, do not."""
    assert own.get_option("fused_keyed") in (0, 1, 2)
    b = C.real(own, corpus, C.chain(5000))
    assert len(b["sigs"][0]) == 10000 and K.reference(b["sigs"][0])[2] == 4
    with Options(own, fused_keyed=0):
        want = own.resolve_batch(**b, seed=9)
    st = own.key_cache_stats(0)
    with Options(own, fused_keyed=1):
        got = own.resolve_batch(**b, seed=9)
        assert sum(moved(own, st)) == 4
        equal(got, want, "auto")
        small = C.real(own, corpus, C.chain(32))
        assert len(small["sigs"][0]) == 64
        st = own.key_cache_stats(0)
        own.resolve_batch(**small, seed=9)
        assert moved(own, st) == (0, 0)


def test_more_keys_than_the_pool_holds_stay_unkeyed(corpus):
    """cv_key_cache_reserve(2) and a batch of four keys under 2: the call stays unkeyed and the pool is not allocated,
    let alone grown; with room for them it takes the keyed route."""
    e = native.Engine(1)
    try:
        e.key_cache_reserve(2)
        b = C.real(e, corpus, C.chain(64))
        with Options(e, fused_keyed=0):
            want = e.resolve_batch(**b, seed=3)
        st = e.key_cache_stats(0)
        with Options(e, fused_keyed=2):
            got = e.resolve_batch(**b, seed=3)
            after = e.key_cache_stats(0)
            assert after == st and after["capacity"] == 0
            equal(got, want, "unkeyed")
            e.key_cache_reserve(4)
            got = e.resolve_batch(**b, seed=3)
            after = e.key_cache_stats(0)
            assert after["misses"] == 4 and after["capacity"] == 4
            equal(got, want, "keyed")
    finally:
        e.close()


# ---------------------------------------------------------------- a repeated bad key
def test_repeated_bad_key_is_the_first_failure(engine, corpus, signer):
    bad = corpus["pk"][corpus["status"] == native.CV_SIG_BAD_KEY][0]
    # resolve: the first signature of transactions 3 and 6 of a chain under one key that is no point
    b = C.real(engine, corpus, C.chain(9))
    pk, sig, tsb, pre = b["sigs"]
    pk[2 * 3] = pk[2 * 6] = bad
    b["reqs"] = b["reqs"][:8] + (pk.copy(),)
    plain, keyed = resolve_both(engine, b, 11)
    equal(plain, keyed, "resolve")
    for t in (3, 6):
        assert keyed["outcome"][t] == native.CV_RS_BAD_KEY and keyed["first_bad"][t] == 2 * t
    # notary: every bad-key transaction of the batch under that one key
    nb = B.make_batch(engine, corpus, 65)
    rows = [int(nb["tx_sig_begin"][t]) for t, k in enumerate(nb["kind"]) if k == "bad_key"]
    assert len(rows) >= 2
    nb["pk"][rows] = bad
    nb["reqs"] = nb["reqs"][:8] + (nb["pk"].copy(),) + nb["reqs"][9:]
    got0, u0 = notarise_under(engine, signer, nb, 0)
    got2, u2 = notarise_under(engine, signer, nb, 2)
    equal(got0, got2, "notary")
    for t, k in enumerate(nb["kind"]):
        if k == "bad_key":
            assert got2["outcome"][t] == native.CV_NS_BAD_KEY and got2["first_bad"][t] == nb["tx_sig_begin"][t]
    u0.close()
    u2.close()
