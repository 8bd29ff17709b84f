"""BatchingNotary(fused=True) — one cv_notarise_batch call per batch — against the default notary, each on its own
fresh provider, over a mixed batch of about 40 requests and a second batch behind it: equal results, field for field.
Restates NotaryServiceTests.kt:46-106 and ValidatingNotaryServiceTests.kt:44-87 for the fused path: good requests, a
missing signer (the notary's own key allowed to be missing), a bad signature, a non-EdDSA key, a key that is no point,
a bad signature length, a tampered id, an empty transaction, an invalid timestamp, a duplicate inside the batch and
one across batches.
"""
import numpy as np
import pytest

import ed25519_ref as E
from corda_amd import native
from corda_amd.crypto import (CompositeKey, DigitalSignature, DummyPublicKey, EdDSAPublicKey, IllegalArgumentException,
                              InvalidKeyException, NullPublicKey)
from corda_amd.notary import (BatchingNotary, Conflict, SignaturesMissing, SignRequest, Timestamp, TimestampChecker,
                              TimestampInvalid, TransactionInvalid)
from corda_amd.transactions import IllegalStateException, MerkleTreeException, SignedTransaction, WireTransaction
from corda_amd.uniqueness import DeviceUniquenessProvider, InMemoryUniquenessProvider

pytestmark = pytest.mark.gpu

NOTARY_SEED = bytes(range(1, 33))
NOW = 1_700_000_000.0


def seed(i):
    return bytes([i % 251 + 1]) * 32


def key(i):
    return EdDSAPublicKey(E.public_key_of(seed(i)))


def make_stx(signers, must=None, inputs=(b"in",), outputs=(b"out",), extra_must=()):
    must = [key(i).composite for i in (signers if must is None else must)] + list(extra_must)
    wtx = WireTransaction(inputs=inputs, outputs=outputs, commands=(b"cmd",), must_sign=must,
                          command_descriptions={m: f"cmd-{j}" for j, m in enumerate(must)})
    txid = wtx.id
    return SignedTransaction(wtx, [DigitalSignature.WithKey(key(i), E.sign(seed(i), txid.bytes)) for i in signers], txid)


def resign(stx, sigs):
    return SignedTransaction(stx._wtx, sigs, stx.id)


def mixed_batch(corpus, notary_key):
    reqs = []
    for i in range(24):                                           # good: 1 to 3 signers, 1 to 3 inputs
        stx = make_stx([10 + i + j for j in range(1 + i % 3)], inputs=[b"good-%d-%d" % (i, j) for j in range(1 + i % 3)])
        reqs.append(SignRequest(stx, f"party{i % 5}", timestamp=Timestamp.around(NOW, 10.0) if i % 4 == 0 else None))
    reqs.append(SignRequest(make_stx([50], must=[50, 51], inputs=(b"s-50",)), "p"))                   # missing signer
    reqs.append(SignRequest(make_stx([52], inputs=(b"s-52",), extra_must=[notary_key]), "p"))         # notary may be missing
    reqs.append(SignRequest(make_stx([53], inputs=(b"s-53",),
                                     extra_must=[CompositeKey.Node(1, [key(53).composite, key(54).composite], [1, 1])]), "p"))
    bad = make_stx([55, 56], inputs=(b"s-55",))
    reqs.append(SignRequest(resign(bad, [bad.sigs[0], DigitalSignature.WithKey(bad.sigs[1].by, b"\x07" * 64)]), "p"))
    nonkey = make_stx([57], inputs=(b"s-57",))
    reqs.append(SignRequest(resign(nonkey, [DigitalSignature.WithKey(NullPublicKey, b"\x00" * 64)] + nonkey.sigs), "p"))
    dummy = make_stx([58], inputs=(b"s-58",))
    reqs.append(SignRequest(resign(dummy, dummy.sigs + [DigitalSignature.WithKey(DummyPublicKey("d"), b"\x01" * 64)]), "p"))
    nopoint = make_stx([59], inputs=(b"s-59",))
    bad_pk = EdDSAPublicKey(corpus["pk"][corpus["status"] == native.CV_SIG_BAD_KEY][0].tobytes())
    reqs.append(SignRequest(resign(nopoint, [DigitalSignature.WithKey(bad_pk, nopoint.sigs[0].bits)] + nopoint.sigs), "p"))
    short = make_stx([60], inputs=(b"s-60",))
    reqs.append(SignRequest(resign(short, [DigitalSignature.WithKey(short.sigs[0].by, b"\x02" * 63)]), "p"))
    stx = make_stx([61], inputs=(b"s-61",))
    other = WireTransaction(inputs=[b"s-61"], outputs=[b"changed"], must_sign=stx._wtx.must_sign)
    reqs.append(SignRequest(SignedTransaction(other, stx.sigs, stx.id), "p"))                       # tampered id
    reqs.append(SignRequest(SignedTransaction(WireTransaction(), stx.sigs, stx.id), "p"))           # empty
    reqs.append(SignRequest(make_stx([62], inputs=(b"s-62",)), "p", timestamp=Timestamp.around(NOW + 3600, 30.0)))
    reqs.append(SignRequest(make_stx([63], inputs=(b"good-3-0", b"s-63"), outputs=(b"dup",)), "double-spender"))
    reqs.append(SignRequest(make_stx([64], inputs=(b"s-62",)), "q"))        # the timestamp failure above committed nothing
    reqs.append(SignRequest(make_stx([65], inputs=(), outputs=(b"issue",)), "q"))                   # no inputs
    reqs.append(SignRequest(make_stx([66], inputs=(b"r", b"r", b"s-66")), "q"))                      # a repeated input
    reqs.append(SignRequest(make_stx([67], inputs=(b"r",), outputs=(b"again",)), "q"))              # conflicts at index 1
    return reqs


def later_batch():
    return [SignRequest(make_stx([70], inputs=(b"good-5-1", b"s-70")), "late"),                      # across batches
            SignRequest(make_stx([71], inputs=(b"s-55",)), "late"),                                 # the bad signature's input
            SignRequest(make_stx([72], inputs=(b"s-72",)), "late")]


def same(a, b, engine):
    assert a.ok == b.ok
    assert (a.sig.bits if a.sig else None) == (b.sig.bits if b.sig else None)
    assert type(a.error) is type(b.error) and type(a.failure) is type(b.failure)
    if isinstance(a.error, SignaturesMissing):
        assert a.error.missing_signers == b.error.missing_signers
    if isinstance(a.error, Conflict):
        ca, cb = a.error.conflict.verified(engine), b.error.conflict.verified(engine)
        assert ca.state_history == cb.state_history and a.error.conflict.raw == b.error.conflict.raw
        assert a.error.conflict.sig.bits == b.error.conflict.sig.bits and a.error.tx is b.error.tx


def test_fused_equals_unfused_on_a_mixed_batch(engine, corpus):
    clock = TimestampChecker(clock=lambda: NOW)
    fused = BatchingNotary(NOTARY_SEED, validating=True, engine=engine, timestamp_checker=clock, fused=True,
                           uniqueness=DeviceUniquenessProvider(engine, capacity=32, leaf_keys=True))
    plain = BatchingNotary(NOTARY_SEED, validating=True, engine=engine, timestamp_checker=clock,
                           uniqueness=InMemoryUniquenessProvider())
    first = mixed_batch(corpus, fused.owning_key)
    assert len(first) >= 40
    for batch in (first, later_batch()):
        got, want = fused.notarise(batch), plain.notarise(batch)
        for a, b in zip(got, want):
            same(a, b, engine)
        if batch is first:
            kinds = [type(r.error or r.failure).__name__ for r in want]
            assert {"SignaturesMissing", "TransactionInvalid", "InvalidKeyException", "IllegalStateException",
                    "MerkleTreeException", "TimestampInvalid", "Conflict", "NoneType"} <= set(kinds)
            assert sum(r.ok for r in want) >= 28 and sum(isinstance(r.error, Conflict) for r in want) == 2
        else:
            assert [r.ok for r in want] == [False, True, True]
    # the provider holds what the sequential one holds, under the leaf-hash key
    assert len(plain.uniqueness.committed) > 40
    for s, c in plain.uniqueness.committed.items():
        assert fused.uniqueness.get(s) == c
    assert fused.notarise([]) == []
    fused.uniqueness.close()


def test_fused_refuses_what_it_cannot_decide(engine):
    prov = DeviceUniquenessProvider(engine, capacity=16, leaf_keys=True)
    with pytest.raises(IllegalArgumentException):
        BatchingNotary(NOTARY_SEED, engine=engine, fused=True)                      # the default provider
    with pytest.raises(IllegalArgumentException):
        BatchingNotary(NOTARY_SEED, engine=engine, fused=True, uniqueness=DeviceUniquenessProvider(engine, capacity=16))
    n = BatchingNotary(NOTARY_SEED, validating=True, engine=engine, fused=True, uniqueness=prov)
    stx = make_stx([80], inputs=(b"s-80",))
    with pytest.raises(IllegalArgumentException):
        n.notarise([SignRequest(stx, "p", input_refs=[b"elsewhere"])])
    odd = make_stx([81], inputs=(b"s-81",), extra_must=[CompositeKey.Leaf(DummyPublicKey("x"))])
    with pytest.raises(IllegalArgumentException):
        n.notarise([SignRequest(odd, "p")])
    assert n.notarise([SignRequest(stx, "p")])[0].ok                                # nothing was committed meanwhile
    simple = BatchingNotary(NOTARY_SEED, validating=False, engine=engine, fused=True, uniqueness=prov)
    assert simple.notarise([SignRequest(odd, "p")])[0].ok                           # the simple notary reads no requirement
    prov.close()
