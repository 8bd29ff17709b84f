"""The uniqueness set on the GPU (cv_uniq_*: the kernels of corda_amd/csrc/cv_k_uniq.hip through the C-ABI and
native.UniquenessSet) against InMemoryUniquenessProvider fed the same requests: the statuses, every conflict's
state -> (id, index, caller) and the lookup of every key ever offered, all EQUAL.  Cases: tests/uniq_cases.py.
Then DeviceUniquenessProvider behind BatchingNotary against the same notary on the in-memory provider.
"""
import numpy as np
import pytest

import ed25519_ref as E
import uniq_cases as C
from corda_amd import native
from corda_amd.crypto import DigitalSignature, EdDSAPublicKey
from corda_amd.notary import BatchingNotary, Conflict, SignRequest, TransactionInvalid
from corda_amd.transactions import SignedTransaction, WireTransaction
from corda_amd.uniqueness import (ConsumingTx, DeviceUniquenessProvider, InMemoryUniquenessProvider,
                                  PersistentUniquenessProvider, UniquenessConflict)

pytestmark = pytest.mark.gpu

DEFAULT_ROUNDS = 8
NAMES = ("tx_status", "state_conflict", "cons_id", "cons_index", "cons_caller")


def _commit(s):
    def run(f):
        return dict(zip(NAMES, s.commit_batch(f["key"], f["begin"], f["id"], f["caller"], f["enable"])))
    return run


@pytest.fixture(scope="module")
def cases():
    return {name: make() for name, make in C.CASES.items()}


@pytest.mark.parametrize("max_rounds", [0, 1, DEFAULT_ROUNDS])
@pytest.mark.parametrize("name", list(C.CASES))
def test_cases_equal_oracle(engine, cases, name, max_rounds):
    """(a)-(f) through cv_uniq_commit_batch with the serial tail alone, one round and the default."""
    with native.UniquenessSet(engine, 4096) as s:
        s.set_max_rounds(max_rounds)
        C.run_case(cases[name], _commit(s), s.lookup, (name, max_rounds))
        st = s.stats()
        if name == "chain":
            assert st["resident"] == 300 and st["rounds"] == max_rounds
            assert st["tail"] == 300 if max_rounds == 0 else st["tail"] > 200      # the default reaches the tail
        if name == "one_key":
            assert st["resident"] == 1
            assert (st["rounds"], st["tail"]) == {0: (0, 1000), 1: (1, 999), DEFAULT_ROUNDS: (2, 0)}[max_rounds]
        if name == "state_counts":
            assert st["resident"] == 1 + 63 + 64 + 65 + 257
        assert st["capacity"] == 4096 and st["slots"] == 8192 and st["probe"] >= 1


def test_default_rounds_and_null_enable(engine):
    """A fresh set runs the default 8 rounds at the most (the chain stops there), and tx_enable = NULL enables all."""
    case = C.chain()
    with native.UniquenessSet(engine, 1024) as s:
        f = C.flatten(case[0])
        got = dict(zip(NAMES, s.commit_batch(f["key"], f["begin"], f["id"], f["caller"], None)))
        C.assert_same(got, C.expect(InMemoryUniquenessProvider(), case[0]))
        assert s.stats()["rounds"] == DEFAULT_ROUNDS


@pytest.mark.parametrize("max_rounds", [0, DEFAULT_ROUNDS])
def test_a_batch_without_states(engine, max_rounds):
    """nstates = 0: all three requests decided (two accepted, the disabled one skipped), nothing resident; the set then
    takes a batch with states as usual."""
    with native.UniquenessSet(engine, 64) as s:
        s.set_max_rounds(max_rounds)
        oracle = C.run_case(C.no_states(), _commit(s), s.lookup, ("no_states", max_rounds))
        assert s.stats()["resident"] == len(oracle.committed) == 1


def test_large_batch(engine):
    """20,000 requests x 2 states with 5 % reuse in one call: many blocks, rounds that end by the device counter."""
    case = C.big_batch()
    with native.UniquenessSet(engine, 1 << 16) as s:
        oracle = C.run_case(case, _commit(s), s.lookup, "big")
        st = s.stats()
        assert st["resident"] == len(oracle.committed) > 30000
        assert 2 <= st["rounds"] <= DEFAULT_ROUNDS


def test_capacity_then_reserve(engine):
    """Open at 64, fill exactly; the next batch is CV_E_OOM with the set and the outputs untouched; reserve 4,096
    (a rehash on the device) and the batch commits as the oracle says."""
    fill = [([C.key_of("cap", 4 * t + j) for j in range(4)], C.tx_id_of("cap", t), t, True) for t in range(16)]
    nxt = [([C.key_of("cap", 64 + t), C.key_of("cap", (7 * t) % 80)], C.tx_id_of("cap", 100 + t), t % 4, t % 9 != 0)
           for t in range(300)]
    keys = C.keys_array(C.all_keys([fill, nxt]))
    oracle = InMemoryUniquenessProvider()
    with native.UniquenessSet(engine, 64) as s:
        C.assert_same(_commit(s)(C.flatten(fill)), C.expect(oracle, fill))
        assert s.stats()["resident"] == 64 == s.stats()["capacity"]
        before = s.lookup(keys)
        f = C.flatten(nxt)
        out = (np.full(300, 0xEE, np.uint8), np.full(600, 0xEE, np.uint8), np.full((600, 32), 0xEE, np.uint8),
               np.full(600, 0xEE, np.uint32), np.full(600, 0xEE, np.uint32))
        with pytest.raises(native.CvError) as ei:
            s.commit_batch(f["key"], f["begin"], f["id"], f["caller"], f["enable"], out=out)
        assert ei.value.code == -4
        assert all((a == 0xEE).all() for a in out)
        for a, b in zip(before, s.lookup(keys)):
            assert np.array_equal(a, b)
        assert s.stats()["resident"] == 64
        s.reserve(4096)
        st = s.stats()
        assert (st["resident"], st["capacity"], st["slots"]) == (64, 4096, 8192)
        for a, b in zip(before, s.lookup(keys)):
            assert np.array_equal(a, b)                                  # every record survived the rehash
        C.assert_same(_commit(s)(f), C.expect(oracle, nxt))
        for g, w in zip(s.lookup(keys), C.expect_lookup(oracle, [k.tobytes() for k in keys])):
            assert np.array_equal(g, w)


def test_load_then_commit(engine):
    """load + commit_batch = the oracle primed with the same rows; a repeated or resident key is CV_E_ARGS and
    leaves the set unchanged."""
    n = 500
    keys = C.keys_array([C.key_of("ld", i) for i in range(n)])
    ids = C.keys_array([C.tx_id_of("ld", i) for i in range(n)])
    index, caller = np.arange(n, dtype=np.uint32) % 4, np.arange(n, dtype=np.uint32) % 7
    oracle = InMemoryUniquenessProvider()
    for i in range(300):
        oracle.committed[keys[i].tobytes()] = ConsumingTx(C.SecureHash(ids[i].tobytes()), int(index[i]), int(caller[i]))
    with native.UniquenessSet(engine, 2048) as s:
        s.load(keys[:300], ids[:300], index[:300], caller[:300])
        assert s.stats()["resident"] == 300
        snap = s.lookup(keys)
        assert snap[0].tolist() == [1] * 300 + [0] * 200 and np.array_equal(snap[1][:300], ids[:300])
        for bad in (np.concatenate([keys[300:400], keys[350:351]]), np.concatenate([keys[400:500], keys[17:18]])):
            with pytest.raises(native.CvError) as ei:
                s.load(bad, ids[:101], index[:101], caller[:101])
            assert ei.value.code == -3
        assert s.stats()["resident"] == 300
        for a, b in zip(snap, s.lookup(keys)):
            assert np.array_equal(a, b)
        batch = [([keys[i].tobytes(), keys[n - 1 - i].tobytes()], C.tx_id_of("ld2", i), i % 5, True) for i in range(0, n, 3)]
        C.assert_same(_commit(s)(C.flatten(batch)), C.expect(oracle, batch))
        for g, w in zip(s.lookup(keys), C.expect_lookup(oracle, [k.tobytes() for k in keys])):
            assert np.array_equal(g, w)


# ---------------------------------------------------------------- behind the notary
def _seed(i):
    return bytes([i % 251 + 1]) * 32


def _stx(i, inputs, bad_sig=False):
    s = _seed(i)
    pk = EdDSAPublicKey(E.public_key_of(s))
    wtx = WireTransaction(inputs=inputs, outputs=(b"out-%d" % i,), commands=(b"cmd",), must_sign=[pk.composite],
                          command_descriptions={pk.composite: f"cmd-{i}"})
    sig = b"\x05" * 64 if bad_sig else E.sign(s, wtx.id.bytes)
    return SignedTransaction(wtx, [DigitalSignature.WithKey(pk, sig)], wtx.id)


def _summary(results):
    out = []
    for r in results:
        if r.ok:
            out.append(("ok", None))
        elif isinstance(r.error, Conflict):
            c = r.error.conflict.verified()
            assert c.serialize() == r.error.conflict.raw
            out.append(("conflict", UniquenessConflict.deserialize(r.error.conflict.raw).state_history))
        else:
            out.append((type(r.error).__name__, None))
    return out


def test_notary_with_device_provider(engine, tmp_path):
    """A first batch, then 64 requests with two double spends (one of a two-input request), one cross-batch
    conflict and one bad signature: the same accepts, conflicts and deserialised conflict reports as the notary on
    InMemoryUniquenessProvider; and the durable log behind the device set restarts it."""
    seed = E.entropy_to_seed(33)
    first = [SignRequest(_stx(200 + i, (b"old-%d" % i,)), f"early{i}") for i in range(4)]
    reqs = []
    for i in range(64):
        inputs = (b"u-%d" % i,)
        if i == 20:
            inputs = (b"u-3",)                               # double spend of request 3
        if i == 41:
            inputs = (b"u-41", b"u-7", b"u-41b")             # double spend of request 7 among fresh inputs
        if i == 50:
            inputs = (b"old-2", b"u-50")                     # consumed by the first batch
        reqs.append(SignRequest(_stx(i, inputs, bad_sig=(i == 30)), f"party{i % 5}"))
    log = PersistentUniquenessProvider(str(tmp_path / "log.db"))
    dev = DeviceUniquenessProvider(engine, capacity=16, log=log)     # small: the provider reserves as it fills
    got_n = BatchingNotary(seed, engine=engine, uniqueness=dev)
    want_n = BatchingNotary(seed, engine=engine, uniqueness=InMemoryUniquenessProvider())
    assert _summary(got_n.notarise(first)) == _summary(want_n.notarise(first)) == [("ok", None)] * 4
    got, want = _summary(got_n.notarise(reqs)), _summary(want_n.notarise(reqs))
    assert got == want
    assert [k for k, (w, _) in enumerate(want) if w == "conflict"] == [20, 41, 50]
    assert want[30][0] == TransactionInvalid.__name__ and sum(w == "ok" for w, _ in want) == 60
    assert list(got[41][1]) == [b"u-7"] and got[41][1][b"u-7"].requesting_party == "party2"
    assert got[50][1][b"old-2"].requesting_party == "early2"
    assert len(dev) == len(want_n.uniqueness.committed) == len(log) == 4 + 60
    # a restart: a new device set warmed from the log decides a late double spend as the in-memory notary does
    dev.close()
    dev2 = DeviceUniquenessProvider(engine, capacity=16, log=log)
    assert len(dev2) == 64
    late = [SignRequest(_stx(300, (b"u-12", b"late-1")), "late")]
    got2 = _summary(BatchingNotary(seed, engine=engine, uniqueness=dev2).notarise(late))
    assert got2 == _summary(want_n.notarise(late)) and got2[0][0] == "conflict"
    assert dev2.get(b"u-12") == want_n.uniqueness.committed[b"u-12"] and dev2.get(b"late-1") is None
    dev2.close()
    log.close()
