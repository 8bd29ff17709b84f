"""The device key store on the GPU (cv_keystore_*, cv_sign_transactions): native.KeyStore and corda_amd.keys against
the Python oracle (oracle/ed25519_ref.py), cv_ed25519_sign_batch with the record's seed, compute_ids and sign_ref
(tests/keystore_cases.py).  The oracle's work — 257 key derivations, 300 signatures, the transactions' signatures — is
done once per module."""
import threading

import numpy as np
import pytest

import ed25519_ref as E
import keystore_cases as K
from corda_amd import native
from corda_amd.crypto import EdDSAPublicKey, IllegalStateException, KeyPair
from corda_amd.keys import DeviceKeyManagementService, InMemoryKeyManagementService, sign_transactions_batch
from corda_amd.transactions import SignedTransaction, WireTransaction, compute_ids, verify_signatures_batch

pytestmark = pytest.mark.gpu

# SHA-512 block crossings of prefix || M and R || A || M (tests/test_sign_keyed_cpu.py), then random up to 300
EDGE_LENGTHS = [0, 1, 32, 47, 48, 79, 80, 143, 144, 175, 176, 300, 1023]
CV_E_OOM = -4


def _rows(list_of_bytes, width=32):
    return np.frombuffer(b"".join(list_of_bytes), np.uint8).reshape(-1, width).copy()


@pytest.fixture(scope="module")
def pool():
    """257 seeds and the oracle's public key of each."""
    rng = np.random.default_rng(2570)
    seeds = [rng.bytes(32) for _ in range(257)]
    return seeds, [E.public_key_of(s) for s in seeds]


@pytest.fixture(scope="module")
def signed(pool):
    """300 records over the first 40 keys of the pool, the key drawn per record, every 16th naming a key the store
    does not hold (pool keys 200..): (key index, message, the oracle's signature or None)."""
    seeds, _ = pool
    rng = np.random.default_rng(300)
    lens = EDGE_LENGTHS + [int(x) for x in rng.integers(0, 301, 300 - len(EDGE_LENGTHS))]
    recs = []
    for i, n in enumerate(lens):
        msg = rng.bytes(n)
        if i % 16 == 15:
            recs.append((200 + int(rng.integers(0, 57)), msg, None))
        else:
            k = int(rng.integers(0, 40))
            recs.append((k, msg, E.sign(seeds[k], msg)))
    return recs


@pytest.fixture(scope="module")
def store40(engine, pool):
    with native.KeyStore(engine, 64) as ks:
        pk, st = ks.add(_rows(pool[0][:40]))
        assert [bytes(r) for r in pk] == pool[1][:40] and not st.any()
        yield ks


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_add_gives_the_oracles_public_keys(engine, pool, n):
    seeds, pks = pool
    with native.KeyStore(engine, n) as ks:
        pk, st = ks.add(_rows(seeds[:n]))
        assert [bytes(r) for r in pk] == pks[:n]
        assert st.tolist() == [K.KS_ADDED] * n
        assert ks.stats()["resident"] == n and ks.contains(_rows(pks[:n])).tolist() == [1] * n
        # the same call again: all PRESENT, nothing more resident (capacity n: the refusal counts repeats, so grow first)
        ks.reserve(2 * n)
        pk, st = ks.add(_rows(seeds[:n]))
        assert [bytes(r) for r in pk] == pks[:n]
        assert st.tolist() == [K.KS_PRESENT] * n
        assert ks.stats()["resident"] == n


def test_add_repeats_in_one_call_first_in_order_wins(engine, pool):
    """130 seeds, 30 of the positions repeating an earlier one: ADDED exactly at first occurrences."""
    seeds, pks = pool
    rng = np.random.default_rng(130)
    order = list(range(100))
    for pos in sorted(int(p) for p in rng.choice(np.arange(1, 130), size=30, replace=False)):
        order.insert(pos, order[int(rng.integers(0, min(pos, len(order))))])
    assert len(order) == 130 and len(set(order)) == 100
    with native.KeyStore(engine, 130) as ks:
        pk, st = ks.add(_rows([seeds[i] for i in order]))
        assert [bytes(r) for r in pk] == [pks[i] for i in order]
        assert st.tolist() == [K.KS_PRESENT if i in order[:j] else K.KS_ADDED for j, i in enumerate(order)]
        assert ks.stats()["resident"] == 100


def _sign_all(ks, pks, msgs):
    arena, offs, lens = native.pack_blobs(msgs)
    return ks.sign(_rows(pks), arena, offs, lens)


def test_capacity_refusal_and_growth(engine, pool):
    seeds, pks = pool
    msgs = [b"message %d" % i for i in range(8)]
    with native.KeyStore(engine, 8) as ks:
        assert ks.stats()["slots"] == 16
        ks.add(_rows(seeds[:8]))
        sig, st = _sign_all(ks, pks[:8], msgs)
        assert not st.any() and [bytes(s) for s in sig] == [E.sign(seeds[i], msgs[i]) for i in range(8)]
        with pytest.raises(native.CvError) as ei:
            ks.add(_rows(seeds[8:9]))
        assert ei.value.code == CV_E_OOM
        assert ks.stats()["resident"] == 8
        assert ks.contains(_rows(pks[:9])).tolist() == [1] * 8 + [0]
        again, st = _sign_all(ks, pks[:8], msgs)
        assert not st.any() and np.array_equal(again, sig)
        ks.reserve(64)
        s = ks.stats()
        assert (s["resident"], s["capacity"], s["slots"]) == (8, 64, 128)
        again, st = _sign_all(ks, pks[:8], msgs)
        assert not st.any() and np.array_equal(again, sig)
        pk, st = ks.add(_rows(seeds[4:40]))
        assert st.tolist() == [K.KS_PRESENT] * 4 + [K.KS_ADDED] * 32 and ks.stats()["resident"] == 40
        again, st = _sign_all(ks, pks[:8], msgs)
        assert not st.any() and np.array_equal(again, sig)


def test_sign_matches_oracle(store40, pool, signed):
    _, pks = pool
    sig, st = _sign_all(store40, [pks[k] for k, _, _ in signed], [m for _, m, _ in signed])
    assert sig.shape == (300, 64)
    for j, (k, m, want) in enumerate(signed):
        if want is None:
            assert st[j] == K.KS_NO_KEY and not sig[j].any(), j
        else:
            assert st[j] == K.KS_OK and sig[j].tobytes() == want, (j, k, len(m))
    assert sum(w is None for _, _, w in signed) == 300 // 16


def test_sign_20003_equals_sign_batch(engine):
    """No multiple of a block (256), many blocks, a 1,000-key store with the key drawn per record: byte-equal to
    sign_batch with the record's seed, and every signature verifies; a one-key store equals Signer.sign."""
    n = 20_003
    rng = np.random.default_rng(20003)
    seeds = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
    which = rng.integers(0, 1000, n)
    lens = rng.integers(0, 120, n).astype(np.uint32)
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    arena = rng.integers(0, 256, int(lens.sum()) + 16, dtype=np.uint8)
    with native.KeyStore(engine, 1000) as ks:
        pk, st = ks.add(seeds)
        assert not st.any()
        sig, st = ks.sign(pk[which], arena, offs, lens)
    want_pk, want = engine.sign_batch(seeds[which], arena, offs, lens)
    assert not st.any() and np.array_equal(want_pk, pk[which]) and np.array_equal(sig, want)
    bitmap, status = engine.verify_batch(pk[which], sig, arena, offs, lens)
    assert native.bitmap_to_bools(bitmap, n).all() and not status.any()
    with native.KeyStore(engine, 1) as one, native.Signer(engine, seeds[7].tobytes()) as signer:
        pk1, _ = one.add(seeds[7:8])
        assert pk1[0].tobytes() == signer.public_key
        sig1, st1 = one.sign(np.tile(pk1, (n, 1)), arena, offs, lens)
        assert not st1.any() and np.array_equal(sig1, signer.sign(arena, offs, lens))


@pytest.fixture(scope="module")
def tx_batch(pool):
    """130 transactions of 0-5 leaves and 0-4 keys over the 40 resident keys — the named precedence cases first, random
    ones behind — with sign_ref's outputs under the oracle's signer."""
    seeds, pks = pool
    rng = np.random.default_rng(1300)
    present, absent = pks[:40], pks[200:]
    cases = K.precedence_txs(present, absent)
    txs = list(cases.values()) + K.random_txs(rng, 130 - len(cases), present, absent)
    want = K.sign_ref({pks[i]: seeds[i] for i in range(40)}, txs, E.sign)
    return txs, want, list(cases)


def test_sign_transactions_equals_sign_ref(engine, store40, tx_batch):
    txs, want, names = tx_batch
    assert len(txs) == 130
    assert [(w[0], w[1]) for w in want[:len(names)]] == [K.PRECEDENCE_EXPECT[n] for n in names]
    assert {w[0] for w in want} == {K.ST_OK, K.ST_NO_KEY, K.ST_ALREADY_SIGNED, K.ST_EMPTY}
    blobs, lb, pk, sb = K.flatten_txs(txs)
    st, ids, sig, fb = store40.sign_transactions(*native.pack_blobs(blobs), lb, pk, sb)
    assert st.tolist() == [w[0] for w in want]
    assert fb.tolist() == [w[1] for w in want]
    assert [bytes(r) for r in ids] == [w[2] for w in want]
    assert [bytes(r) for r in sig] == [s for w in want for s in w[3]]
    got_ids = compute_ids([WireTransaction(commands=leaves) for leaves, _ in txs], engine)
    assert [bytes(32) if g is None else g.bytes for g in got_ids] == [bytes(r) for r in ids]


def _same(a, b):
    if isinstance(a, Exception) or isinstance(b, Exception):
        return type(a) is type(b) and str(a) == str(b)
    return a.id == b.id and [(s.by, s.bits) for s in a.sigs] == [(s.by, s.bits) for s in b.sigs]


def test_python_paths_agree_and_signed_transactions_verify(engine, pool, tx_batch):
    """sign_transactions_batch fused and composed, over the device service and the in-memory one: equal results,
    exceptions included; the transactions that come out signed pass verify_signatures_batch."""
    seeds, pks = pool
    txs, want, _ = tx_batch
    wtxs = lambda: [WireTransaction(commands=leaves) for leaves, _ in txs]  # noqa: E731
    keys = [[EdDSAPublicKey(k) for k in ks] for _, ks in txs]
    with DeviceKeyManagementService(engine, 16, initial_seeds=seeds[:40]) as dev:
        assert dev.keys == {EdDSAPublicKey(k) for k in pks[:40]}
        assert EdDSAPublicKey(pks[3]) in dev and EdDSAPublicKey(pks[200]) not in dev
        fused = sign_transactions_batch(wtxs(), keys, dev, fused=True)
        composed = sign_transactions_batch(wtxs(), keys, dev, fused=False)
        mem = InMemoryKeyManagementService(engine, initial_seeds=seeds[:40])
        host = sign_transactions_batch(wtxs(), keys, mem, fused=False)
        mem.close()
        # sign_many: the first absent key in order raises; sign of one record equals the key pair's
        with pytest.raises(IllegalStateException, match="No private key known for requested public key"):
            dev.sign_many([(EdDSAPublicKey(pks[0]), b"a"), (EdDSAPublicKey(pks[201]), b"b"), (EdDSAPublicKey(pks[202]), b"c")])
        kp = KeyPair(seeds[5], engine)
        assert dev.sign(kp.public, b"hello").bits == kp.sign_with_ecdsa(b"hello").bits == E.sign(seeds[5], b"hello")
        kp.close()
    for t, (f, c, h, w) in enumerate(zip(fused, composed, host, want)):
        assert _same(f, c) and _same(f, h), (t, f, c, h)
        if w[0] == K.ST_OK and w[3]:
            assert isinstance(f, SignedTransaction) and f.id.bytes == w[2] and [s.bits for s in f.sigs] == w[3], t
        else:
            assert isinstance(f, Exception), t
    ok = [f for f in fused if isinstance(f, SignedTransaction)]
    assert len(ok) >= 20 and verify_signatures_batch(ok, engine=engine) == [None] * len(ok)


def test_eight_threads_sign_while_a_ninth_adds(engine, pool, signed):
    """Eight threads sign their slices of the oracle's records over one store, ten times each, while a ninth adds
    unrelated keys: every signature and every public key is the oracle's."""
    seeds, pks = pool
    errors = []
    with native.KeyStore(engine, 256) as ks:
        ks.add(_rows(seeds[:40]))

        def sign_slice(w):
            try:
                mine = signed[w::8]
                for _ in range(10):
                    sig, st = _sign_all(ks, [pks[k] for k, _, _ in mine], [m for _, m, _ in mine])
                    for j, (_, _, want) in enumerate(mine):
                        if (sig[j].tobytes(), st[j]) != ((bytes(64), K.KS_NO_KEY) if want is None else (want, K.KS_OK)):
                            errors.append(("sign", w, j))
            except Exception as e:  # noqa: BLE001 - reported below
                errors.append(("sign", w, repr(e)))

        def add_more():
            try:
                for b in range(40, 200, 16):
                    pk, st = ks.add(_rows(seeds[b:b + 16]))
                    if [bytes(r) for r in pk] != pks[b:b + 16] or st.any():
                        errors.append(("add", b))
            except Exception as e:  # noqa: BLE001
                errors.append(("add", repr(e)))

        threads = [threading.Thread(target=sign_slice, args=(w,)) for w in range(8)] + [threading.Thread(target=add_more)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors[:5]
        assert ks.stats()["resident"] == 200
        # the records that named absent keys (pool keys 200..) are still refused; the added ones sign
        assert ks.contains(_rows(pks)).tolist() == [1] * 200 + [0] * 57
