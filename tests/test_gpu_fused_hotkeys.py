"""CV_OPT_FUSED_KEYED 3 and 4 on the GPU: cv_resolve_batch and cv_notarise_batch with their verify handed to the hot-key
route — as tests/test_gpu_fused_keyed.py for 2: every case of tests/resolve_cases.py at its sizes and
every group of tests/notarise_cases.py under 0 and 4, every output equal array for array between the two and equal to
the reference over the component calls.  One resolve batch and one notary batch whose keys are mixed — a pool beside
keys that sign once — with cv_key_cache_stats, on engines of this module's own, showing that only the hot keys were
looked up; auto (3) takes the route above the tri-chain size only; the option's range ends at 4.
"""
import numpy as np
import pytest

import hotkeys_cases as H
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
    """Array for array; of a resolve call's graph the words resolve_cases.same compares (the other two are the join
    table's longest probe and its wraps, which depend on which lane claimed a slot first)."""
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = (a[k][:C.G_COMPARED], b[k][:C.G_COMPARED]) if k == "graph" else (a[k], b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), (what, k)


def moved(engine, before):
    st = engine.key_cache_stats(0)
    return st["hits"] - before["hits"], st["misses"] - before["misses"]


def notarise_under(engine, signer, b, mode):
    """A fresh set per setting, so the commits match."""
    uniq = B.open_set(engine, b)
    with Options(engine, fused_keyed=mode):
        got = B.call(engine, uniq, signer, b)
    return got, uniq


def resolve_both(engine, b, seed, mode=4):
    with Options(engine, fused_keyed=0):
        plain = engine.resolve_batch(**b, seed=seed)
    with Options(engine, fused_keyed=mode):
        hot = engine.resolve_batch(**b, seed=seed)
    return plain, hot


@pytest.mark.parametrize("n", C.SIZES)
def test_resolve_cases_under_0_and_4(engine, corpus, n):
    ran = 0
    for name, build in C.CASES.items():
        specs = build(n)
        if specs is None:
            continue
        b = C.real(engine, corpus, specs)
        txs, ids, req_missing = C.components(engine, b)
        want = C.resolve_ref(txs)
        plain, hot = resolve_both(engine, b, 1 + ran)
        equal(plain, hot, (name, n))
        C.same(hot, want, (name, n))
        assert np.array_equal(hot["ids"], ids) and np.array_equal(hot["req_missing"], req_missing), (name, n)
        ran += 1
    assert ran >= 5


@pytest.fixture(scope="module")
def signer(engine):
    s = native.Signer(engine, B.NOTARY_SEED)
    yield s
    s.close()


@pytest.mark.parametrize("name", list(NC.CASES))
def test_notary_groups_under_0_and_4(engine, corpus, signer, name):
    txs, resident = NC.CASES[name]()
    b, plain = notarise_real.realise(engine, corpus, txs, resident)
    want, ref_set = B.compose(engine, signer, b)
    keys = np.concatenate([B.state_keys(b), b["resident"][0]])
    got = {}
    for mode in (0, 4):
        got[mode], uniq = notarise_under(engine, signer, b, mode)
        for k in NOTARY_NAMES:
            assert got[mode][k].shape == want[k].shape and np.array_equal(got[mode][k], want[k]), (name, mode, k)
        assert B.same_sets(uniq, ref_set, keys), (name, mode)
        uniq.close()
    equal(got[0], got[4], name)
    ref_set.close()


# ---------------------------------------------------------------- mixed keys: only the hot ones are looked up
def resign(engine, pk, sig, rows, msgs, tag):
    """Signatures `rows` again, each under a key of its own, over msgs[j] (32 bytes each)."""
    seeds = K.pool(("own seeds", tag), len(rows))
    arena = np.ascontiguousarray(msgs, np.uint8).reshape(-1)
    p, s = engine.sign_batch(seeds, arena, (np.arange(len(rows)) * 32).astype(np.uint64), np.full(len(rows), 32, np.uint32))
    pk[rows], sig[rows] = p, s


def test_resolve_mixed_keys(corpus):
    """chain(64): 128 signatures under the four keys of resolve_cases._signed; the first signature of every third
    transaction signed again under a key of its own.  Under 4 the pool of four is hot, the others cold."""
    e = native.Engine(1)
    try:
        e.key_cache_reserve(64)
        specs = C.chain(64)
        b = C.real(e, corpus, specs)
        pk, sig, tsb, pre = b["sigs"]
        ids = np.frombuffer(b"".join(C.real_leaves(specs)[2]), np.uint8).reshape(-1, 32)
        txs = np.arange(0, 64, 3)
        resign(e, pk, sig, 2 * txs, ids[txs], "resolve")
        b["reqs"] = b["reqs"][:8] + (pk.copy(),)
        nkeys, hot_keys, hot, cold = H.route(pk, 2, 64)
        assert (nkeys, hot_keys, cold) == (4 + len(txs), 4, len(txs)) and hot == 128 - len(txs)
        txs_ref, ids_ref, req_missing = C.components(e, b)
        want = C.resolve_ref(txs_ref)
        st = e.key_cache_stats(0)
        plain, got = resolve_both(e, b, 21)
        assert moved(e, st) == (0, 4)                          # one lookup a hot key, none for the keys that sign once
        equal(plain, got, "mixed")
        C.same(got, want, "mixed")
        assert (got["outcome"] == plain["outcome"]).all() and np.array_equal(got["ids"], ids_ref)
        with Options(e, fused_keyed=4):
            again = e.resolve_batch(**b, seed=21)
        assert moved(e, st) == (4, 4)
        equal(got, again, "mixed again")
        with Options(e, fused_keyed=3):                        # auto: 128 signatures stay below the tri-chain size
            e.resolve_batch(**b, seed=21)
        assert moved(e, st) == (4, 4)
    finally:
        e.close()


def test_resolve_auto_takes_a_long_chain(corpus):
    """3: a chain of 5,000 transactions — 10,000 signatures, four keys — takes the route, every key hot."""
    e = native.Engine(1)
    try:
        e.key_cache_reserve(64)
        b = C.real(e, corpus, C.chain(5000))
        with Options(e, fused_keyed=0):
            want = e.resolve_batch(**b, seed=9)
        st = e.key_cache_stats(0)
        with Options(e, fused_keyed=3):
            got = e.resolve_batch(**b, seed=9)
        assert moved(e, st) == (0, 4)
        equal(got, want, "auto")
    finally:
        e.close()


def test_notary_mixed_keys(corpus):
    """make_batch(65): a pool of eight keys and the bad keys, once each; the last signature of some accepted
    transactions signed again under a key of its own.  Under 4 only the keys that sign twice or more are looked up."""
    e = native.Engine(1)
    e.key_cache_reserve(64)
    signer = native.Signer(e, B.NOTARY_SEED)
    sets = []
    try:
        b = B.make_batch(e, corpus, 65)
        tsb = b["tx_sig_begin"]
        txs = np.array([t for t, k in enumerate(b["kind"]) if k == "success" and t % 4 != 1 and tsb[t + 1] - tsb[t] >= 2])
        assert len(txs) >= 3
        resign(e, b["pk"], b["sig"], tsb[txs + 1] - 1, b["claimed"][txs], "notary")
        b["reqs"] = b["reqs"][:8] + (b["pk"].copy(),) + b["reqs"][9:]
        nkeys, hot_keys, hot, cold = H.route(b["pk"], 2, 64)
        assert 0 < hot_keys <= 8 and cold >= len(txs) + 2 and nkeys > hot_keys
        want, ref_set = B.compose(e, signer, b)
        sets.append(ref_set)
        st = e.key_cache_stats(0)
        got0, u = notarise_under(e, signer, b, 0)
        sets.append(u)
        assert moved(e, st) == (0, 0)
        got4, u = notarise_under(e, signer, b, 4)
        sets.append(u)
        assert moved(e, st) == (0, hot_keys)
        equal(got0, got4, "notary 0 against 4")
        for k in NOTARY_NAMES:
            assert np.array_equal(got4[k], want[k]), k
        assert (got4["outcome"][txs] == want["outcome"][txs]).all()
        got4b, u = notarise_under(e, signer, b, 4)
        sets.append(u)
        assert moved(e, st) == (hot_keys, hot_keys)
        equal(got4, got4b, "notary 4 again")
    finally:
        for u in sets:
            u.close()
        signer.close()
        e.close()


def test_option_range(engine):
    old = engine.get_option("fused_keyed")
    try:
        for v in (3, 4):
            engine.set_option("fused_keyed", v)
            assert engine.get_option("fused_keyed") == v
        with pytest.raises(native.CvError) as err:
            engine.set_option("fused_keyed", 5)
        assert err.value.code == -3                            # CV_E_ARGS
        assert engine.get_option("fused_keyed") == 4
    finally:
        engine.set_option("fused_keyed", old)
