"""Fixed-key batch signing on the GPU (cv_signer, cv_ed25519_sign_keyed): native.Signer, crypto.KeyPair and the
notary's reply signatures against the Python oracle, today's sign_batch and the engine's own verify."""
import ctypes

import numpy as np
import pytest

import ed25519_ref as E
from corda_amd import native
from corda_amd.crypto import DigitalSignature, EdDSAPublicKey, KeyPair, SignatureException, verify_with_ecdsa
from corda_amd.notary import BatchingNotary, Conflict, SignRequest
from corda_amd.transactions import SignedTransaction, WireTransaction, compute_ids

pytestmark = pytest.mark.gpu

SEED_A = E.entropy_to_seed(20)                 # DUMMY_NOTARY_KEY
SEED_B = E.entropy_to_seed(10)                 # DUMMY_CASH_ISSUER_KEY
# SHA-512 block crossings of prefix || M and R || A || M (tests/test_sign_keyed_cpu.py), then random up to 300
EDGE_LENGTHS = [0, 1, 32, 47, 48, 79, 80, 143, 144, 175, 176, 300, 1023]
CV_E_ARGS = -3


def _pack(msgs):
    lens = np.fromiter((len(m) for m in msgs), np.uint32, count=len(msgs))
    offs = np.zeros(len(msgs), np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(msgs) + b"\0" * 16, np.uint8), offs, lens


def _all_ok(engine, pk32: bytes, sigs, arena, offs, lens):
    n = len(offs)
    bitmap, status = engine.verify_batch(np.tile(np.frombuffer(pk32, np.uint8), (n, 1)), sigs, arena, offs, lens)
    return native.bitmap_to_bools(bitmap, n).all() and not status.any()


@pytest.fixture(scope="module")
def pool():
    """1,000 ragged messages and their oracle signatures under SEED_A, computed once for the module."""
    rng = np.random.default_rng(2016)
    lens = EDGE_LENGTHS + [int(x) for x in rng.integers(0, 301, 1000 - len(EDGE_LENGTHS))]
    msgs = [rng.bytes(n) for n in lens]
    return msgs, [E.sign(SEED_A, m) for m in msgs]


@pytest.fixture(scope="module")
def signer_a(engine):
    with native.Signer(engine, SEED_A) as s:
        yield s


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_sign_matches_oracle(engine, signer_a, pool, n):
    msgs, want = pool[0][:n], pool[1][:n]
    arena, offs, lens = _pack(msgs)
    sigs = signer_a.sign(arena, offs, lens)
    assert sigs.shape == (n, 64)
    assert signer_a.public_key == E.public_key_of(SEED_A)
    for j in range(n):
        assert sigs[j].tobytes() == want[j], (j, len(msgs[j]))
    assert _all_ok(engine, signer_a.public_key, sigs, arena, offs, lens)


def test_sign_20003_equals_sign_batch(engine, signer_a):
    """No multiple of a block (256) or a shard unit (64), many blocks: byte-equal to sign_batch with the seed
    repeated, and every signature verifies."""
    n = 20_003
    rng = np.random.default_rng(20003)
    lens = rng.integers(0, 120, n).astype(np.uint32)
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    arena = rng.integers(0, 256, int(lens.sum()) + 16, dtype=np.uint8)
    sigs = signer_a.sign(arena, offs, lens)
    pk, want = engine.sign_batch(np.tile(np.frombuffer(SEED_A, np.uint8), (n, 1)), arena, offs, lens)
    assert np.array_equal(sigs, want)
    assert pk[0].tobytes() == pk[-1].tobytes() == signer_a.public_key
    assert _all_ok(engine, signer_a.public_key, sigs, arena, offs, lens)


def test_two_signers_alternate(engine, signer_a, pool):
    """Two keys in one process, a call of one between two calls of the other: each output is its own key's."""
    msgs = pool[0][:40]
    arena, offs, lens = _pack(msgs)
    want_b = [E.sign(SEED_B, m) for m in msgs]
    with native.Signer(engine, SEED_B) as signer_b:
        assert signer_b.public_key == E.public_key_of(SEED_B) != signer_a.public_key
        for s, want in ((signer_a, pool[1]), (signer_b, want_b), (signer_a, pool[1]), (signer_b, want_b)):
            got = s.sign(arena, offs, lens)
            assert [g.tobytes() for g in got] == list(want[:40])


def test_threads_share_one_signer(engine, signer_a, pool):
    """A signer is immutable after open: eight threads signing with it at once each get the oracle's bytes."""
    from concurrent.futures import ThreadPoolExecutor
    n = 300
    arena, offs, lens = _pack(pool[0][:n])
    want = np.frombuffer(b"".join(pool[1][:n]), np.uint8).reshape(n, 64)

    def work(_):
        return all(np.array_equal(signer_a.sign(arena, offs, lens), want) for _ in range(3))

    with ThreadPoolExecutor(8) as ex:
        assert all(ex.map(work, range(8)))


def test_batch_cut_over_device_slots(engine, pool):
    """A context with three device slots on the one GPU (cv_open_ex): the signer holds a record per slot, and a
    batch cut over the slots (spread_min = 64: shards in multiples of 64) is the oracle's, message for message."""
    msgs, want = pool
    arena, offs, lens = _pack(msgs)
    ve = native.Engine(1, virtual_devices=3)
    try:
        ve.set_option("spread_min", 64)
        with native.Signer(ve, SEED_A) as s:
            assert s.public_key == E.public_key_of(SEED_A)
            ve.stats("route", reset=True)
            sigs = s.sign(arena, offs, lens)
            route = ve.stats("route")
        assert route["split_calls"] == 1 and route["shards"] == 3
        assert [g.tobytes() for g in sigs] == list(want)
    finally:
        ve.close()


def test_device_form_is_stream_ordered(engine, signer_a, pool):
    """sign_device on a non-default stream, then verify_device on the same stream over the signatures it produces,
    no host synchronise in between: an all-ones bitmap, and the oracle's bytes."""
    import torch
    n = 640
    msgs = pool[0][:n]
    arena, offs, lens = _pack(msgs)
    dev = "cuda:0"
    d_arena = torch.from_numpy(arena.copy()).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_pk = torch.from_numpy(np.tile(np.frombuffer(signer_a.public_key, np.uint8), (n, 1))).to(dev)
    d_sig = torch.full((n, 64), 0xAB, dtype=torch.uint8, device=dev)
    d_bm = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    signer_a.sign_device(0, n, d_arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_sig.data_ptr(),
                         stream.cuda_stream)
    engine.verify_device(0, n, d_pk.data_ptr(), d_sig.data_ptr(), d_arena.data_ptr(), d_off.data_ptr(),
                         d_len.data_ptr(), d_bm.data_ptr(), 0, stream.cuda_stream)
    stream.synchronize()
    assert bool((d_bm == -1).all())
    got = d_sig.cpu().numpy()
    assert [g.tobytes() for g in got] == list(pool[1][:n])


def test_argument_checks(engine, signer_a):
    lib, ctx, sg = engine._lib, engine._h, signer_a._h
    arena = np.zeros(64, np.uint8)
    off = np.array([0, 10], np.uint64)
    ln = np.array([10, 54], np.uint32)
    poison = np.full((2, 64), 0x5A, np.uint8)
    p = native._p

    def call(n, a, abytes, o, l, out):
        return lib.cv_ed25519_sign_keyed(ctx, sg, n, a, abytes, o, l, out)

    out = poison.copy()
    assert call(0, p(arena), 64, p(off), p(ln), p(out)) == 0              # n = 0: nothing touched
    assert call(0, None, 0, None, None, None) == 0
    assert np.array_equal(out, poison)
    assert call(2, p(arena), 64, None, p(ln), p(out)) == CV_E_ARGS        # null arrays
    assert call(2, p(arena), 64, p(off), None, p(out)) == CV_E_ARGS
    assert call(2, p(arena), 64, p(off), p(ln), None) == CV_E_ARGS
    assert call(2, None, 64, p(off), p(ln), p(out)) == CV_E_ARGS
    assert lib.cv_ed25519_sign_keyed(ctx, None, 2, p(arena), 64, p(off), p(ln), p(out)) == CV_E_ARGS
    assert call(2, p(arena), 64, p(off), p(ln), p(out)) == 0               # exactly to the arena's end
    assert not np.array_equal(out, poison)
    out = poison.copy()
    assert call(2, p(arena), 63, p(off), p(ln), p(out)) == CV_E_ARGS      # one byte past msg_arena_bytes
    ln2 = np.array([10, 55], np.uint32)
    assert call(2, p(arena), 64, p(off), p(ln2), p(out)) == CV_E_ARGS
    wrap = np.array([0, (1 << 64) - 8], np.uint64)                          # off + len wraps
    assert call(2, p(arena), 64, p(wrap), p(ln), p(out)) == CV_E_ARGS
    assert call(2, p(arena), (1 << 64) - 1, p(wrap), p(ln), p(out)) == CV_E_ARGS
    assert np.array_equal(out, poison)
    with pytest.raises(ValueError):
        signer_a.sign(arena, off, ln2)
    # the device form's checks
    assert lib.cv_ed25519_sign_keyed_device(ctx, 0, sg, 0, None, None, None, None, None) == 0
    assert lib.cv_ed25519_sign_keyed_device(ctx, 0, sg, 2, None, None, None, None, None) == CV_E_ARGS
    assert lib.cv_ed25519_sign_keyed_device(ctx, 0, None, 2, 16, 16, 16, 16, None) == CV_E_ARGS
    assert lib.cv_signer_public_key(None, p(arena)) == CV_E_ARGS
    assert lib.cv_signer_open(ctx, None, ctypes.byref(ctypes.c_void_p())) == CV_E_ARGS
    assert lib.cv_signer_close(None) is None


def test_signer_reopen(engine, pool):
    """open -> close -> open with the same seed: the same key, the same signatures."""
    arena, offs, lens = _pack(pool[0][:70])
    first = native.Signer(engine, SEED_B)
    pk1, s1 = first.public_key, first.sign(arena, offs, lens)
    first.close()
    first.close()                                                           # idempotent
    with pytest.raises(ValueError):
        first.sign(arena, offs, lens)
    with native.Signer(engine, SEED_B) as again:
        assert again.public_key == pk1 == E.public_key_of(SEED_B)
        assert np.array_equal(again.sign(arena, offs, lens), s1)
    assert s1[12].tobytes() == E.sign(SEED_B, pool[0][12])


def test_key_pair_round_trip(engine):
    kp = KeyPair.from_entropy(10, engine)
    assert kp.public == EdDSAPublicKey(E.public_key_of(SEED_B))
    sig = kp.sign_with_ecdsa(b"\x00\x01\x02\x03")
    assert isinstance(sig, DigitalSignature.WithKey) and sig.by == kp.public
    assert sig.bits == E.sign(SEED_B, b"\x00\x01\x02\x03")
    verify_with_ecdsa(kp.public, b"\x00\x01\x02\x03", sig, engine)
    with pytest.raises(SignatureException, match="Signature did not match"):
        verify_with_ecdsa(kp.public, b"\x00\x01\x02\x04", sig, engine)
    msgs = [bytes([i]) * i for i in range(1, 30)]
    many = kp.sign_many(msgs)
    assert kp.sign_many([]) == []
    for m, s in zip(msgs, many):
        verify_with_ecdsa(kp.public, m, s, engine)
    assert many[4].bits == E.sign(SEED_B, msgs[4])
    with pytest.raises(SignatureException):
        verify_with_ecdsa(kp.public, msgs[3], many[4], engine)
    kp.close()


def test_notary_replies_signed_with_the_keyed_signer(engine):
    """BatchingNotary over 64 requests, every fourth spending an input an earlier request spent: each Result.sig
    and each Conflict's SignedData verifies under notary.public_key and equals the oracle's signature."""
    seed = E.entropy_to_seed(21)
    notary = BatchingNotary(seed, validating=False, engine=engine)
    assert notary.public_key.encoded == E.public_key_of(seed)
    wtxs = [WireTransaction(inputs=(b"state-%d" % (k - 1 if k % 4 == 3 else k),), outputs=(b"out-%d" % k,),
                            commands=(b"cmd",)) for k in range(64)]
    compute_ids(wtxs, engine)
    anyone = EdDSAPublicKey(E.public_key_of(SEED_B))
    reqs = [SignRequest(SignedTransaction(w, [DigitalSignature.WithKey(anyone, b"\x01" * 64)], w.id), f"party{k}")
            for k, w in enumerate(wtxs)]
    res = notary.notarise(reqs)
    nconf = 0
    for k, r in enumerate(res):
        if k % 4 == 3:
            assert isinstance(r.error, Conflict)
            sd = r.error.conflict
            assert sd.sig.by == notary.public_key and sd.sig.bits == E.sign(seed, sd.raw)
            sd.verified(engine)
            nconf += 1
        else:
            assert r.ok and r.sig.by == notary.public_key
            assert r.sig.bits == E.sign(seed, reqs[k].stx.id.bytes)
            verify_with_ecdsa(notary.public_key, reqs[k].stx.id.bytes, r.sig, engine)
    assert nconf == 16
