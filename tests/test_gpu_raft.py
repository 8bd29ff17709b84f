"""corda_amd/raft.py on the device: the scenarios of tests/raft_scenarios.py (tests/test_raft_cpu.py runs them on
dicts) with three DeviceBackend replicas that differ in capacity and max_rounds — so in table size, growth and in how a
batch is decided — and a DictBackend replica as the witness: InProcessCluster.submit raises when a replica's answer
differs from the leader's, and the scenarios compare every replica's map.  Then one BatchingNotary batch through
RaftUniquenessProvider on the notary's default path against the same batch through DeviceUniquenessProvider.
"""
import pytest

import ed25519_ref as E
import raft_scenarios as R
from corda_amd import native
from corda_amd.crypto import DigitalSignature, EdDSAPublicKey
from corda_amd.notary import BatchingNotary, Conflict, SignRequest
from corda_amd.raft import DeviceBackend, DictBackend, DistributedImmutableMap, InProcessCluster, RaftUniquenessProvider
from corda_amd.transactions import SignedTransaction, WireTransaction
from corda_amd.uniqueness import DeviceUniquenessProvider

pytestmark = pytest.mark.gpu

SHAPES = ((16, 0), (1024, 1), (1 << 14, 8))        # (capacity, max_rounds) of the three device replicas


def device_machine(engine, capacity, max_rounds):
    s = native.UniquenessSet(engine, capacity)
    s.set_max_rounds(max_rounds)
    return DistributedImmutableMap(DeviceBackend(s))


def machines(engine):
    """Three device replicas (the first leads) and the dict witness."""
    return [device_machine(engine, c, r) for c, r in SHAPES] + [DistributedImmutableMap(DictBackend())]


def test_replicas_decide_as_the_sequential_provider(engine):
    R.replicas_decide_as_the_sequential_provider(machines(engine)).close()


def test_one_entry_decides_as_one_command_at_a_time(engine):
    """The one-by-one side is the dict's (hundreds of single-command entries); the one-entry side the device's."""
    R.one_entry_decides_as_one_command_at_a_time(machines(engine), [DistributedImmutableMap(DictBackend())])


def test_compaction_join_and_catch_up(engine):
    """The late joiner is a device replica that installs a device snapshot; the witness joins last, from a later one."""
    R.compaction_join_and_catch_up(machines(engine)[:3], device_machine(engine, 64, 2),
                                   extra=DistributedImmutableMap(DictBackend())).close()


def _seed(i):
    return bytes([i % 251 + 1]) * 32


def _requests(n=40):
    """n signed transactions of 1-3 inputs (tests/test_gpu_uniq.py's shape); every fifth spends an input an earlier one
    spends, among fresh ones."""
    reqs, spent = [], []
    for t in range(n):
        ins = [b"state-%d-%d" % (t, j) for j in range(1 + t % 3)]
        if t % 5 == 4:
            ins[-1] = spent[(t // 5) % 7]                # an input of requests 0-3, which are accepted
        spent.extend(ins)
        s = _seed(t)
        pk = EdDSAPublicKey(E.public_key_of(s))
        wtx = WireTransaction(inputs=ins, outputs=(b"out-%d" % t,), commands=(b"cmd",), must_sign=[pk.composite],
                              command_descriptions={pk.composite: f"cmd-{t}"})
        stx = SignedTransaction(wtx, [DigitalSignature.WithKey(pk, E.sign(s, wtx.id.bytes))], wtx.id)
        reqs.append(SignRequest(stx, f"party-{t % 4}"))
    return reqs


def _content(results):
    """A Result's whole content as plain values: the notary's signature bytes and key, or the error's type with the
    signed conflict report's bytes and signature, or the failure."""
    out = []
    for r in results:
        if r.ok:
            out.append(("ok", r.sig.bytes, r.sig.by))
        elif isinstance(r.error, Conflict):
            r.error.conflict.verified()
            out.append(("conflict", r.error.tx.id, r.error.conflict.raw, r.error.conflict.sig.bytes, r.error.conflict.sig.by))
        else:
            out.append((type(r.error).__name__, repr(r.failure)))
    return out


def test_batching_notary_on_a_replicated_set(engine):
    """The same Result objects (content for content: signatures are deterministic) from
    BatchingNotary(uniqueness=RaftUniquenessProvider) on its default, non-fused path as from the same notary on a
    DeviceUniquenessProvider."""
    reqs, seed = _requests(), E.entropy_to_seed(33)
    cluster = InProcessCluster(machines(engine))
    plain = DeviceUniquenessProvider(engine, 1024)
    try:
        got = _content(BatchingNotary(seed, engine=engine, uniqueness=RaftUniquenessProvider(cluster)).notarise(reqs))
        want = _content(BatchingNotary(seed, engine=engine, uniqueness=plain).notarise(reqs))
        assert got == want
        assert [k for k, w in enumerate(want) if w[0] == "conflict"] == list(range(4, 40, 5))
        assert sum(w[0] == "ok" for w in want) == 32
        R.same_state(cluster)
        assert cluster.leader().machine.size() == len(plain)
    finally:
        cluster.close()
        plain.close()
