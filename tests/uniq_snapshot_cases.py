"""Shared cases of the snapshot / clear / install tests of the uniqueness set (tests/test_uniq_snapshot_cpu.py on the
CPU harness, tests/test_gpu_uniq_snapshot.py on the device) and their oracle: a plain dict, key bytes -> (id bytes,
index, caller), the literal DistributedImmutableMap (DistributedImmutableMap.kt:24-106).

A set under test is anything with the calls of native.UniquenessSet: load, commit_batch-style commits are the test
files' own; here only snapshot(max_entries=None) -> (key (n,32) u8, id (n,32) u8, index u32[n], caller u32[n]),
snapshot_chunks(max_entries) -> a generator of such chunks, and lookup(keys).  Everything is seeded: the cases are the
same in every process.
"""
import numpy as np

import uniq_cases as C

CHUNKS = (7, 64, 65, 256, 257, 1000)      # max_entries of the chunked passes over the larger sets
WRAP_SEED = 5                             # tests/test_uniq_cpu.py: with it a probe of the 8 "w" keys passes slot 15


def entries(n, seed):
    """n distinct random entries: (key (n,32) u8, id (n,32) u8, index u32[n], caller u32[n])."""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    assert len({k.tobytes() for k in key}) == n
    return key, rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 1 << 32, n, dtype=np.uint32), \
        rng.integers(0, 1 << 32, n, dtype=np.uint32)


def wrap_entries():
    """The 8 keys of tests/test_uniq_cpu.py's wrap test, one request each: a batch for C.flatten and its entries."""
    keys = [C.key_of("w", i) for i in range(8)]
    batch = [([k], C.tx_id_of("w", i), 100 + i, True) for i, k in enumerate(keys)]
    e = (C.keys_array(keys), C.keys_array([C.tx_id_of("w", i) for i in range(8)]), np.zeros(8, np.uint32),
         np.arange(100, 108, dtype=np.uint32))
    return batch, e


def model_of(*parts):
    """The dict model of one or more entry tuples."""
    m = {}
    for key, cid, cix, cc in parts:
        for j in range(len(key)):
            m[key[j].tobytes()] = (cid[j].tobytes(), int(cix[j]), int(cc[j]))
    return m


def as_model(snap):
    """A snapshot's arrays as the dict model; every key once."""
    key, cid, cix, cc = snap
    assert key.shape == (len(cix), 32) and cid.shape == key.shape and cix.dtype == np.uint32 and len(cc) == len(cix)
    m = model_of(snap)
    assert len(m) == len(key), "a key reported twice"
    return m


def same_bytes(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def check_passes(s, model, chunks=CHUNKS, what=""):
    """One whole pass equals the model as a set; a second pass and every chunked pass equal it byte for byte, no chunk
    is longer than asked for.  Returns the one-call pass."""
    one = s.snapshot()
    assert as_model(one) == model, what
    assert same_bytes(s.snapshot(), one), (what, "second pass")
    for m in chunks:
        parts = list(s.snapshot_chunks(m))
        assert all(len(p[2]) <= m for p in parts), (what, m)
        if parts:
            got = tuple(np.concatenate([p[j] for p in parts]) for j in range(4))
            assert same_bytes(got, one), (what, m)
        else:
            assert len(one[2]) == 0
    return one


def check_lookups(s, model, absent):
    """Every key of the model is found with its record, every key of `absent` (keys (k,32)) is not."""
    keys = C.keys_array(list(model)) if model else np.zeros((0, 32), np.uint8)
    if len(keys):
        found, cid, cix, cc = s.lookup(keys)
        assert found.all()
        assert model_of((keys, cid, cix, cc)) == model
    found, cid, cix, cc = s.lookup(absent)
    assert not found.any() and not cid.any() and not cix.any() and not cc.any()


def follow_up(model_keys, n=120, seed=99):
    """A commit batch for C.flatten over a set holding model_keys (a list of key bytes): about a third of the
    requests spend a resident key, some spend a key an earlier request of the batch spends, the rest are fresh."""
    import random
    rng = random.Random(seed)
    batch, fresh = [], []
    for t in range(n):
        ks = [C.key_of("fu", 3 * t + j) for j in range(rng.randrange(1, 4))]
        r = rng.random()
        if model_keys and r < 0.33:
            ks.insert(rng.randrange(len(ks) + 1), rng.choice(model_keys))
        elif fresh and r < 0.5:
            ks.append(rng.choice(fresh))
        fresh.extend(ks)
        batch.append((ks, C.tx_id_of("fu", t), t % 7, True))
    return batch
