"""The outputs of the key store's five calls that have any (cv_keystore_add, _contains, _sign, _stats,
cv_sign_transactions) under the header's Conventions (include/cordaverify.h): every output carved out of poisoned,
guard-banded buffers (tests/guarded.py) at the contract's minimum alignment — bytes for keys, signatures, ids and
statuses, 4 for first_bad, 8 for the statistics — n = 65 records and nsig = 65 signatures.  A successful call writes
every byte of every output it is given, whatever they held, and nothing around them; signatures are zero exactly where
the header says; a call that fails (CV_E_OOM, CV_E_ARGS) writes nothing."""
import numpy as np
import pytest

import keystore_cases as K
from corda_amd import native
from guarded import Guarded

pytestmark = pytest.mark.gpu

N = 65
FILLS = (0x00, 0xA5, 0xFF)
P = native._p


@pytest.fixture(scope="module")
def material(engine):
    """65 seeds, their keys and signatures from cv_ed25519_sign_batch, and a second set the store never sees."""
    rng = np.random.default_rng(65)
    seeds = rng.integers(0, 256, (2 * N, 32), dtype=np.uint8)
    msgs = rng.integers(0, 256, 2 * N * 40, dtype=np.uint8)
    off, ln = np.arange(2 * N, dtype=np.uint64) * 40, np.full(2 * N, 40, np.uint32)
    pk, sig = engine.sign_batch(seeds, msgs, off, ln)
    return dict(seeds=seeds, pk=pk, sig=sig, msgs=msgs, off=off, ln=ln)


@pytest.fixture(scope="module")
def store(engine, material):
    with native.KeyStore(engine, N) as ks:
        ks.add(material["seeds"][:N])
        yield ks


def _whole(g, what):
    g.check_guards(str(what))


def test_add_writes_all_of_pk_out_and_status(engine, material):
    m = material
    for fill in FILLS:
        g = Guarded([("pk", 32 * N, 1), ("status", N, 1)], fill)
        with native.KeyStore(engine, 2 * N) as ks:
            assert ks._lib.cv_keystore_add(ks._h, N, P(m["seeds"]), g.ptr("pk"), g.ptr("status")) == 0
            _whole(g, ("add", hex(fill)))
            assert np.array_equal(g.read("pk").reshape(N, 32), m["pk"][:N])
            assert g.read("status").tolist() == [K.KS_ADDED] * N
            g.refill()
            assert ks._lib.cv_keystore_add(ks._h, N, P(m["seeds"]), g.ptr("pk"), g.ptr("status")) == 0
            _whole(g, ("add again", hex(fill)))
            assert np.array_equal(g.read("pk").reshape(N, 32), m["pk"][:N])
            assert g.read("status").tolist() == [K.KS_PRESENT] * N
            # past the capacity (130 + 65), a null array, an empty call: nothing written
            g.refill()
            assert ks._lib.cv_keystore_add(ks._h, N, P(m["seeds"][N:]), g.ptr("pk"), g.ptr("status")) == 0
            g.refill()
            assert ks._lib.cv_keystore_add(ks._h, N, P(m["seeds"]), g.ptr("pk"), g.ptr("status")) == -4
            assert ks._lib.cv_keystore_add(ks._h, N, None, g.ptr("pk"), g.ptr("status")) == -3
            assert ks._lib.cv_keystore_add(ks._h, N, P(m["seeds"]), g.ptr("pk"), None) == -3
            assert ks._lib.cv_keystore_add(ks._h, 0, P(m["seeds"]), g.ptr("pk"), g.ptr("status")) == 0
            _whole(g, ("add refused", hex(fill)))
            assert g.untouched("pk") and g.untouched("status")
            assert ks.stats()["resident"] == 2 * N


def test_contains_and_stats(store, material):
    m = material
    ask = np.concatenate([m["pk"][:33], m["pk"][N:N + 32]])            # 33 resident, 32 absent
    for fill in FILLS:
        g = Guarded([("found", N, 1), ("stats", 8 * 6, 8)], fill)
        assert store._lib.cv_keystore_contains(store._h, N, P(ask), g.ptr("found")) == 0
        assert store._lib.cv_keystore_stats(store._h, g.ptr("stats"), 6) == 0
        _whole(g, ("contains", hex(fill)))
        assert g.read("found").tolist() == [1] * 33 + [0] * 32
        st = g.read("stats", np.uint64).tolist()
        assert st[:3] == [N, N, 256] and st[3] >= 1 and st[4:] == [0, 0]       # entries past the count: zero
        g.refill()
        assert store._lib.cv_keystore_contains(store._h, N, None, g.ptr("found")) == -3
        assert store._lib.cv_keystore_contains(store._h, 0, P(ask), g.ptr("found")) == 0
        assert store._lib.cv_keystore_stats(None, g.ptr("stats"), 6) == -3
        assert store._lib.cv_keystore_stats(store._h, g.ptr("stats"), 0) == 0
        _whole(g, ("contains refused", hex(fill)))
        assert g.untouched("found") and g.untouched("stats")


def test_sign_zero_signatures_exactly_for_absent_keys(store, material):
    m = material
    absent = np.zeros(N, bool)
    absent[[0, 7, 63, 64]] = True
    pk = np.where(absent[:, None], m["pk"][N:], m["pk"][:N])
    for fill in FILLS:
        g = Guarded([("sig", 64 * N, 1), ("status", N, 1)], fill)

        def call(n=N, bound=m["msgs"].size, pkp=P(pk), sig="sig"):
            return store._lib.cv_keystore_sign(store._h, n, pkp, P(m["msgs"]), bound, P(m["off"]), P(m["ln"]),
                                               g.ptr(sig) if sig else None, g.ptr("status"))

        assert call() == 0
        _whole(g, ("sign", hex(fill)))
        sig = g.read("sig").reshape(N, 64)
        assert g.read("status").tolist() == [K.KS_NO_KEY if a else K.KS_OK for a in absent]
        assert not sig[absent].any() and np.array_equal(sig[~absent], m["sig"][:N][~absent])
        g.refill()
        assert call(bound=40 * N - 1) == -3                             # the last record ends past the arena
        assert call(pkp=None) == -3
        assert call(sig=None) == -3
        assert call(n=0) == 0
        _whole(g, ("sign refused", hex(fill)))
        assert g.untouched("sig") and g.untouched("status")


def test_sign_transactions_outputs(engine, store, material):
    """65 signatures over 40 transactions: every status occurs; abandoned transactions' signatures are zero, the
    others' are their keys' signatures over the id; ids of transactions without leaves are zero."""
    m = material
    present, absent = [r.tobytes() for r in m["pk"][:N]], [r.tobytes() for r in m["pk"][N:]]
    rng = np.random.default_rng(6500)
    txs = list(K.precedence_txs(present, absent).values())
    while sum(len(ks) for _, ks in txs) < N:
        txs.extend(K.random_txs(rng, 1, present, absent))
    over = sum(len(ks) for _, ks in txs) - N
    txs[-1] = (txs[-1][0], txs[-1][1][:len(txs[-1][1]) - over])
    seed_of = {p: m["seeds"][i] for i, p in enumerate(present)}

    def sign(seed, msg):
        _, s = engine.sign_batch(seed[None, :], np.frombuffer(msg, np.uint8), np.zeros(1, np.uint64), np.array([len(msg)], np.uint32))
        return s[0].tobytes()

    want = K.sign_ref(seed_of, txs, sign)
    assert {w[0] for w in want} == {K.ST_OK, K.ST_NO_KEY, K.ST_ALREADY_SIGNED, K.ST_EMPTY}
    blobs, lb, pk, sb = K.flatten_txs(txs)
    arena, off, ln = native.pack_blobs(blobs)
    T = len(txs)
    assert len(pk) == N
    for fill in FILLS:
        g = Guarded([("tx_status", T, 1), ("ids", 32 * T, 1), ("sig", 64 * N, 1), ("first_bad", 4 * T, 4)], fill)

        def call(ntx=T, bound=arena.size, sbp=sb, fbad="first_bad", ids="ids"):
            return store._lib.cv_sign_transactions(engine._h, store._h, ntx, P(arena), bound, P(off), P(ln), P(lb), N, P(pk),
                                                   P(sbp), g.ptr("tx_status"), g.ptr(ids) if ids else None, g.ptr("sig"),
                                                   g.ptr(fbad) if fbad else None)

        assert call() == 0
        _whole(g, ("sign_transactions", hex(fill)))
        assert g.read("tx_status").tolist() == [w[0] for w in want]
        assert g.read("first_bad", np.uint32).tolist() == [w[1] for w in want]
        assert [bytes(r) for r in g.read("ids").reshape(T, 32)] == [w[2] for w in want]
        assert [bytes(r) for r in g.read("sig").reshape(N, 64)] == [s for w in want for s in w[3]]
        g.refill()
        assert call(fbad=None) == 0                                     # optional: left alone, the rest written
        _whole(g, ("without first_bad", hex(fill)))
        assert g.untouched("first_bad") and g.read("tx_status").tolist() == [w[0] for w in want]
        g.refill()
        leaves_end = int(off[int(lb[-1]) - 1] + ln[int(lb[-1]) - 1])
        assert call(bound=leaves_end - 1) == -3                         # the last leaf ends past the arena
        short = sb.copy()
        short[-1] -= 1
        assert call(sbp=short) == -3                                    # ends short of nsig
        assert call(ids=None) == -3
        assert call(ntx=0) == 0
        _whole(g, ("sign_transactions refused", hex(fill)))
        assert all(g.untouched(k) for k in ("tx_status", "ids", "sig", "first_bad"))
