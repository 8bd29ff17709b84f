"""Shared cases of the uniqueness-set tests (tests/test_uniq_cpu.py on the CPU harness, tests/test_gpu_uniq.py on
the device) and their oracle: InMemoryUniquenessProvider of corda_amd/uniqueness.py fed the same requests.

A case is a list of batches committed one after another into ONE set; a batch is a list of requests
(keys, tx_id, caller, enabled): keys a list of 32-byte state keys, tx_id 32 bytes, caller a u32 handle.  `flatten`
gives the arrays the C-ABI takes, `expect` the arrays it must give back, `expect_lookup` what a lookup over every key
ever offered must find afterwards.  Everything is seeded: the cases are the same in every process.
"""
import hashlib
import random

import numpy as np

from corda_amd.transactions import SecureHash
from corda_amd.uniqueness import InMemoryUniquenessProvider

OK, CONFLICT, SKIPPED = 0, 1, 2


def key_of(tag, i) -> bytes:
    return hashlib.sha256(f"{tag}:{i}".encode()).digest()


def tx_id_of(tag, i) -> bytes:
    return hashlib.sha256(f"tx:{tag}:{i}".encode()).digest()


# ---------------------------------------------------------------- (a) - (f)
def reference_scenarios():
    """(a) UniquenessProviderTests.kt restated as tests/test_uniqueness.py restates it: a commit of unused inputs;
    the same inputs again -> a conflict naming the consuming id, index and party; a conflicting commit is all or
    nothing ([b, a, c] fails on a alone, [b, c] is then accepted).  One request per batch, as the reference commits."""
    s, a, b, c = (key_of("a", i) for i in range(4))
    return [[([s], tx_id_of("a", 0), 7, True)],
            [([s], tx_id_of("a", 0), 7, True)],
            [([a], tx_id_of("a", 1), 1, True)],
            [([b, a, c], tx_id_of("a", 2), 2, True)],
            [([b, c], tx_id_of("a", 3), 3, True)]]


def random_carry_over(seed=20161019):
    """(b) 4 batches of 300 requests on one set, 0-5 states each from a pool of 200 keys (heavy reuse inside a batch
    and across batches), some states repeated inside a request, empty requests, about 10 % disabled."""
    rng = random.Random(seed)
    pool = [key_of("b", i) for i in range(200)]
    case = []
    for bi in range(4):
        batch = []
        for t in range(300):
            keys = [rng.choice(pool) for _ in range(rng.randrange(6))]
            if keys and rng.random() < 0.2:
                keys.insert(rng.randrange(len(keys) + 1), rng.choice(keys))      # a state repeated in the request
            batch.append((keys, tx_id_of("b", 300 * bi + t), rng.randrange(5), rng.random() >= 0.1))
        case.append(batch)
    return case


def chain(n=300):
    """(c) request t holds keys t and t + 1: sequentially every other request is accepted (150 of 300), and a
    parallel round decides only the head of the chain."""
    return [[([key_of("c", t), key_of("c", t + 1)], tx_id_of("c", t), t % 3, True) for t in range(n)]]


def one_key(n=1000):
    """(d) every request spends the same key: the first alone is accepted."""
    k = key_of("d", 0)
    return [[([k], tx_id_of("d", t), t, True) for t in range(n)]]


def near_keys():
    """(e) keys equal in their first 28 bytes and different in the last word, and keys different in byte 0 only:
    all distinct states, one request each, then each once more (conflicts with exactly its own record)."""
    base = key_of("e", 0)
    keys = [base[:28] + bytes([i, 0, 0, 0]) for i in range(8)] + [base[:31] + bytes([0x80 | i]) for i in range(4)]
    keys += [bytes([i]) + base[1:] for i in range(8)]
    assert len(set(keys)) == len(keys) == 20
    first = [([k], tx_id_of("e", i), i, True) for i, k in enumerate(keys)]
    again = [([k], tx_id_of("e", 100 + i), 50 + i, True) for i, k in enumerate(keys)]
    return [first + again]


def state_counts():
    """(f) requests of 1, 63, 64, 65 and 257 distinct states, then one request per size that repeats each one's
    last state among fresh ones (a conflict on exactly that state)."""
    sizes = [1, 63, 64, 65, 257]
    batch, nk = [], 0
    lasts = []
    for j, n in enumerate(sizes):
        keys = [key_of("f", nk + i) for i in range(n)]
        nk += n
        lasts.append(keys[-1])
        batch.append((keys, tx_id_of("f", j), j, True))
    for j, n in enumerate(sizes):
        keys = [key_of("f", nk + i) for i in range(n)]
        nk += n
        keys[n // 2] = lasts[j]
        batch.append((keys, tx_id_of("f", 10 + j), 10 + j, True))
    return [batch]


CASES = {"reference": reference_scenarios, "random": random_carry_over, "chain": chain, "one_key": one_key,
         "near_keys": near_keys, "state_counts": state_counts}


def no_states():
    """A batch whose requests have no states at all (nstates = 0: every state-sized piece of the call's workspace is
    empty), one of them disabled, then a batch with states on the same set.  Not in CASES: nothing is ever probed."""
    return [[([], tx_id_of("h", t), t, t != 1) for t in range(3)],
            [([key_of("h", 0)], tx_id_of("h", 3), 3, True), ([], tx_id_of("h", 4), 4, True),
             ([key_of("h", 0), key_of("h", 1)], tx_id_of("h", 5), 5, True)]]


def big_batch(ntx=20000, seed=7):
    """20,000 requests x 2 states with 5 % reuse: a state is, with probability 0.05, one an earlier request used."""
    rng = random.Random(seed)
    used, batch, fresh = [], [], 0
    for t in range(ntx):
        keys = []
        for _ in range(2):
            if used and rng.random() < 0.05:
                keys.append(rng.choice(used))
            else:
                keys.append(key_of("g", fresh))
                fresh += 1
        used.extend(keys)
        batch.append((keys, tx_id_of("g", t), t % 11, True))
    return [batch]


# ---------------------------------------------------------------- arrays in, arrays out
def flatten(batch):
    """-> dict(ntx, nstates, key (S,32) u8, begin u32[ntx+1], id (ntx,32) u8, caller u32[ntx], enable u8[ntx])."""
    keys = [k for ks, _, _, _ in batch for k in ks]
    begin = np.concatenate([[0], np.cumsum([len(ks) for ks, _, _, _ in batch])]).astype(np.uint32)
    return dict(ntx=len(batch), nstates=len(keys),
                key=np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32).copy(),
                begin=begin,
                id=np.frombuffer(b"".join(i for _, i, _, _ in batch), np.uint8).reshape(-1, 32).copy(),
                caller=np.array([c for _, _, c, _ in batch], np.uint32),
                enable=np.array([1 if e else 0 for _, _, _, e in batch], np.uint8))


def expect(oracle: InMemoryUniquenessProvider, batch):
    """The batch through the oracle (its enabled requests, in order, in ONE commit_batch) -> dict(tx_status,
    state_conflict, cons_id, cons_index, cons_caller), zero where the C-ABI writes zero."""
    f = flatten(batch)
    enabled = [(t, r) for t, r in enumerate(batch) if r[3]]
    decided = oracle.commit_batch([(list(ks), SecureHash(i), c) for _, (ks, i, c, _) in enabled])
    st = np.full(f["ntx"], SKIPPED, np.uint8)
    sc = np.zeros(f["nstates"], np.uint8)
    cid = np.zeros((f["nstates"], 32), np.uint8)
    cix = np.zeros(f["nstates"], np.uint32)
    cc = np.zeros(f["nstates"], np.uint32)
    for (t, (ks, _, _, _)), d in zip(enabled, decided):
        st[t] = OK if d is None else CONFLICT
        if d is None:
            continue
        assert d.state_history
        for j, k in enumerate(ks):
            c = d.state_history.get(k)
            if c is not None:
                i = int(f["begin"][t]) + j
                sc[i], cix[i], cc[i] = 1, c.input_index, c.requesting_party
                cid[i] = np.frombuffer(c.id.bytes, np.uint8)
    return dict(tx_status=st, state_conflict=sc, cons_id=cid, cons_index=cix, cons_caller=cc)


def all_keys(case):
    """Every key the case ever offers, each once, in first-offer order."""
    seen = {}
    for batch in case:
        for ks, _, _, _ in batch:
            for k in ks:
                seen.setdefault(k, None)
    return list(seen)


def expect_lookup(oracle: InMemoryUniquenessProvider, keys):
    """-> (found u8[n], id (n,32) u8, index u32[n], caller u32[n]) of the oracle's map for these keys."""
    n = len(keys)
    found, cid = np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
    cix, cc = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i, k in enumerate(keys):
        c = oracle.committed.get(k)
        if c is not None:
            found[i], cix[i], cc[i] = 1, c.input_index, c.requesting_party
            cid[i] = np.frombuffer(c.id.bytes, np.uint8)
    return found, cid, cix, cc


def keys_array(keys):
    return np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32).copy()


def assert_same(got: dict, want: dict, what=""):
    for name in ("tx_status", "state_conflict", "cons_id", "cons_index", "cons_caller"):
        assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), (what, name)


def run_case(case, commit, lookup, what=""):
    """Commits the case's batches through commit(flat) -> dict and compares each with the oracle; then lookup(keys
    (n,32)) -> (found, id, index, caller) over every key ever offered against the oracle's map.  Returns the oracle."""
    oracle = InMemoryUniquenessProvider()
    for bi, batch in enumerate(case):
        want = expect(oracle, batch)
        assert_same(commit(flatten(batch)), want, (what, bi))
    keys = all_keys(case)
    if keys:
        got = lookup(keys_array(keys))
        for g, w, name in zip(got, expect_lookup(oracle, keys), ("found", "id", "index", "caller")):
            assert np.array_equal(g, w), (what, "lookup", name)
    return oracle
