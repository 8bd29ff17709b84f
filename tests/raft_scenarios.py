"""The scenarios of the replicated uniqueness provider (corda_amd/raft.py), written once over DistributedImmutableMap
machines of any backend: tests/test_raft_cpu.py runs them on DictBackends, tests/test_gpu_raft.py on DeviceBackends
with a DictBackend witness.  The batches are tests/uniq_cases.py's, as provider requests (states, tx id, caller name).
"""
import uniq_cases as C
from corda_amd.raft import InProcessCluster, PutAll, RaftUniquenessProvider
from corda_amd.transactions import SecureHash
from corda_amd.uniqueness import InMemoryUniquenessProvider


def requests_of(batch):
    """A uniq_cases batch's enabled requests as CommitRequests; the states are the raw 32-byte values."""
    return [(list(ks), SecureHash(i), f"party-{c}") for ks, i, c, on in batch if on]


def batches():
    """Random batches with heavy reuse, the chain, near keys and requests of many states: all on ONE set."""
    return [requests_of(b) for b in C.random_carry_over() + C.chain(120) + C.near_keys() + C.state_counts() + C.one_key(50)]


def contents_of(snapshot):
    key, cid, cix, cc = snapshot.arrays()
    return {key[j].tobytes(): (cid[j].tobytes(), int(cix[j]), snapshot.parties[int(cc[j])]) for j in range(len(cix))}


def same_state(cluster):
    """Every live replica holds the same map and party table as the leader and answers size alike."""
    lead = cluster.leader().machine
    want = lead.contents()
    for i, r in enumerate(cluster.replicas):
        if r.live:
            assert r.machine.size() == lead.size() == len(want), i
            assert r.machine.parties == lead.parties, i
            assert r.machine.contents() == want, i
    return want


def replicas_decide_as_the_sequential_provider(machines):
    """Every replica returns the leader's conflicts, and every decision equals InMemoryUniquenessProvider.commit_batch
    on the same requests."""
    cluster = InProcessCluster(machines)
    provider, oracle = RaftUniquenessProvider(cluster), InMemoryUniquenessProvider()
    conflicts = accepted = 0
    for reqs in batches():
        got, want = provider.commit_batch(reqs), oracle.commit_batch(reqs)
        assert got == want
        conflicts += sum(c is not None for c in got)
        accepted += sum(c is None for c in got)
        for i in range(len(machines)):
            assert cluster.results(i) == cluster.results(0), i
    assert conflicts > 100 and accepted > 100
    assert len(provider) == len(oracle.committed)
    same_state(cluster)
    for s, c in list(oracle.committed.items())[:50]:
        assert provider.get(s) == c
    assert provider.get(b"\x00" * 32) is None
    # the single commit: accepted, then the conflict the reference raises
    from corda_amd.uniqueness import UniquenessException
    import pytest
    s1, tx = C.key_of("single", 0), SecureHash(C.tx_id_of("single", 0))
    provider.commit([s1], tx, "party-x")
    with pytest.raises(UniquenessException) as ei:
        provider.commit([C.key_of("single", 1), s1], SecureHash(C.tx_id_of("single", 1)), "party-y")
    assert list(ei.value.error.state_history) == [s1] and ei.value.error.state_history[s1].requesting_party == "party-x"
    return cluster


def one_entry_decides_as_one_command_at_a_time(machines_a, machines_b):
    """A batch submitted as one log entry decides exactly as the same commands submitted one by one."""
    a, b = InProcessCluster(machines_a), InProcessCluster(machines_b)
    for reqs in batches()[:3]:
        cmds = [PutAll(tuple(RaftUniquenessProvider._key(s) for s in states), t.bytes, c) for states, t, c in reqs]
        whole = a.submit(cmds)
        single = [b.submit([cmd])[0] for cmd in cmds]
        assert whole == single
    assert a.last == 3 and b.last > 600
    assert same_state(a) == same_state(b)


def compaction_join_and_catch_up(machines, late, extra=None):
    """compact() truncates the log; a replica that joins late installs the snapshot and replays the tail; a stopped
    replica catches up by replay, and by install once its log position has been compacted away.  `extra`: a
    machine that joins an uncompacted-then-compacted cluster last (the GPU run passes its witness here)."""
    cluster = InProcessCluster(machines)
    provider, oracle = RaftUniquenessProvider(cluster), InMemoryUniquenessProvider()
    bs = batches()

    def run(k):
        assert provider.commit_batch(bs[k]) == oracle.commit_batch(bs[k])

    run(0)
    run(1)
    cluster.stop(2)                                   # replica 2 misses entries 3 and 4
    run(2)
    run(3)
    assert cluster.replicas[2].applied == 2 and cluster.last == 4
    assert cluster.restart(2) == "replay"
    same_state(cluster)
    cluster.stop(1)                                   # replica 1 misses entry 5, then the log before 6 goes
    run(4)
    assert cluster.compact() == 5 and cluster.first == 6 and cluster.log == []
    run(5)
    assert cluster.first == 6 and cluster.last == 6 and len(cluster.log) == 1
    n = cluster.join(late)                            # installs the snapshot (entry 5), replays entry 6
    assert cluster.replicas[n].applied == 6
    assert cluster.restart(1) == "install"
    assert cluster.replicas[1].applied == 6
    want = same_state(cluster)
    assert len(want) == len(oracle.committed)
    for r in cluster.replicas:
        for s, c in list(oracle.committed.items())[:20]:
            assert r.machine.get(RaftUniquenessProvider._key(s)) == (c.id.bytes, c.input_index, c.requesting_party)
        assert r.machine.get(b"\x01" * 32) is None
    run(6)                                            # and the cluster goes on deciding as the oracle
    if extra is not None:
        cluster.compact()
        cluster.join(extra)
        run(7)
    same_state(cluster)
    return cluster
