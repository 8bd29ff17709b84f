"""corda_amd/raft.py on DictBackends: the cluster logic of the replicated uniqueness provider (DistributedImmutableMap.kt:
24-106, RaftUniquenessProvider.kt:106-115) with no GPU.  tests/raft_scenarios.py holds the scenarios, which
tests/test_gpu_raft.py runs again on device replicas; here too the Snapshot file format.
"""
import numpy as np
import pytest

import raft_scenarios as R
from corda_amd.crypto import IllegalArgumentException
from corda_amd.raft import DictBackend, DistributedImmutableMap
from corda_amd.uniqueness import Snapshot


def machines(n=3):
    return [DistributedImmutableMap(DictBackend()) for _ in range(n)]


def fresh():
    return DistributedImmutableMap(DictBackend())


def test_replicas_decide_as_the_sequential_provider():
    R.replicas_decide_as_the_sequential_provider(machines())


def test_one_entry_decides_as_one_command_at_a_time():
    R.one_entry_decides_as_one_command_at_a_time(machines(), machines())


def test_compaction_join_and_catch_up():
    R.compaction_join_and_catch_up(machines(), fresh())


def test_put_is_the_reference_put():
    """DistributedImmutableMap.put (:59-72) on one machine: all or nothing, the conflicts are the stored entries, a
    repeated key keeps its last index."""
    from corda_amd.raft import PutAll
    m = fresh()
    a, b, c = (bytes([i]) * 32 for i in (1, 2, 3))
    assert m.put(PutAll((a, b, a), b"\x11" * 32, "alice")) == {} and m.size() == 2
    assert m.get(a) == (b"\x11" * 32, 2, "alice") and m.get(b) == (b"\x11" * 32, 1, "alice") and m.get(c) is None
    assert m.put(PutAll((c, a), b"\x22" * 32, "bob")) == {a: (b"\x11" * 32, 2, "alice")}
    assert m.size() == 2 and m.get(c) is None                 # nothing of a conflicting command is stored
    assert m.put(PutAll((), b"\x33" * 32, "bob")) == {}
    assert m.parties == ["alice", "bob"]


def _snapshot():
    ms = machines(1)
    R.replicas_decide_as_the_sequential_provider(ms)
    s = ms[0].snapshot()
    assert len(s) > 100 and len(s.parties) > 1
    return s


def test_snapshot_file_round_trip(tmp_path):
    s = _snapshot()
    path = str(tmp_path / "uniq.snap")
    s.write(path)
    t = Snapshot.read(path)
    assert t.parties == s.parties and t.leaf_keys == s.leaf_keys
    for a, b in zip(t.arrays(), s.arrays()):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    m = fresh()
    m.install(t)
    assert m.contents() == R.contents_of(s) and m.size() == len(s)
    empty = Snapshot.from_bytes(fresh().snapshot().to_bytes())
    assert len(empty) == 0 and empty.parties == []


def test_snapshot_file_refuses_a_corrupted_byte(tmp_path):
    raw = _snapshot().to_bytes()
    for at in (0, 9, 20, 40, len(raw) // 2, len(raw) - 33, len(raw) - 1):
        bad = bytearray(raw)
        bad[at] ^= 0x40
        with pytest.raises(IllegalArgumentException):
            Snapshot.from_bytes(bytes(bad))
    for cut in (raw[:-1], raw[:40], b""):
        with pytest.raises(IllegalArgumentException):
            Snapshot.from_bytes(cut)
    path = str(tmp_path / "bad.snap")
    bad = bytearray(raw)
    bad[len(raw) // 3] ^= 1
    with open(path, "wb") as f:
        f.write(bytes(bad))
    with pytest.raises(IllegalArgumentException):
        Snapshot.read(path)
