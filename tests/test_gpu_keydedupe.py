"""cv_ed25519_dedupe_keys_device on the GPU (corda_amd/csrc/cv_keydedupe.h, cv_k_dedupe.hip) against first-seen
numbering in plain Python (tests/keydedupe_cases.py): the cases of the CPU test, then the sizes at which the kernels
take another path — one below, at and one above CV_BLOCK (256, a lane kernel's block) and the compaction's block span
(CVD_SPAN = 1024: one block, then a level of block sums), and one above the next level's boundary (1024^2 rows, a
second level of sums; the boundary after that, 1024^3, is past what a test allocates).  Every output lies poisoned
between guard bands (tests/guarded.py) at the contract's minimum alignment: rows of d_keys from nkeys on and the guards
keep their poison.  The last test feeds the result to cv_ed25519_verify_device_keyed.
"""
import numpy as np
import pytest
import torch

import keydedupe_cases as C
from guarded import DEVICE_ALIGN, Guarded
from corda_amd import native

pytestmark = pytest.mark.gpu

POISON = 0xA7
DEV = "cuda:0"


def dedupe(engine, pk):
    """-> (keys[:nkeys], key_index, nkeys) through guarded, poisoned outputs; checks what must stay untouched."""
    n = len(pk)
    d_pk = torch.from_numpy(np.ascontiguousarray(pk, np.uint8)).to(DEV)
    ws = torch.full((native.dedupe_keys_workspace(n),), 0x5C, dtype=torch.uint8, device=DEV)   # nothing is expected in it
    g = Guarded([("d_keys", 32 * n, DEVICE_ALIGN["d_keys"]), ("d_key_index", 4 * n, DEVICE_ALIGN["d_key_index"]),
                 ("d_nkeys", 4, 4)], POISON, device=DEV)
    torch.cuda.synchronize()
    engine.dedupe_keys_device(0, n, d_pk.data_ptr(), g.ptr("d_keys"), g.ptr("d_key_index"), g.ptr("d_nkeys"), ws.data_ptr())
    engine.synchronize(0)
    g.snapshot()
    g.check_guards(f"n={n}")
    nk = int(g.read("d_nkeys", np.uint32)[0])
    assert 1 <= nk <= n, nk
    keys = g.read("d_keys", np.uint8, (n, 32))
    assert (keys[nk:] == POISON).all(), "a row of d_keys past nkeys was written"
    return keys[:nk], g.read("d_key_index", np.uint32), nk


def same(got, want, what):
    assert got[2] == want[2], (what, got[2], want[2])
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what


@pytest.fixture(scope="module")
def cases():
    return {name: (pk, C.reference(pk)) for name, pk in C.cases().items()}


@pytest.mark.parametrize("name", list(C.cases()))
def test_cases_equal_the_reference(engine, cases, name):
    pk, want = cases[name]
    same(dedupe(engine, pk), want, name)


@pytest.mark.parametrize("n", (255, 256, 257, 1023, 1024, 1025, 2049))
def test_block_and_span_boundaries(engine, n):
    """A pool of 97 keys and, in the second half, keys of their own: first occurrences on both sides of every block."""
    rng = np.random.default_rng(n)
    pk = C.pool("span", 97)[rng.integers(0, 97, n)].copy()
    fresh = np.flatnonzero(rng.integers(0, 3, n) == 0)
    fresh = fresh[fresh >= n // 2]
    pk[fresh] = C.pool(("own", n), len(fresh))
    pk[n - 1] = C.key("last", n)                       # a first occurrence in the last lane
    want = C.reference(pk)
    assert want[2] > 97
    same(dedupe(engine, pk), want, n)


def test_all_distinct_past_one_span(engine):
    """Every flag set over three blocks of the compaction: the ranks are the indices."""
    rng = np.random.default_rng(5)
    pk = rng.integers(0, 256, (2500, 32), dtype=np.uint8)
    want = C.reference(pk)
    assert want[2] == 2500
    same(dedupe(engine, pk), want, "distinct")


def test_second_level_of_block_sums(engine):
    """One row past 1024^2: the block sums themselves take more than one block.  A pool of 8 keys, the last of them
    first seen in the last row, and a run of one key across the boundary."""
    n = (1 << 20) + 1
    pool = C.pool("level", 8)
    pk = pool[np.random.default_rng(9).integers(0, 7, n)].copy()
    pk[-1] = pool[7]
    want = C.reference(pk)
    assert want[2] == 8 and want[1][-1] == 7
    same(dedupe(engine, pk), want, n)


def test_two_calls_one_result(engine, cases):
    """The table's seed is drawn per process, not per call; the result is a function of the bytes: a second call into
    fresh buffers, and a call on the rows reversed, give what the reference gives."""
    pk, want = cases["signed_pool_of_4"]
    same(dedupe(engine, pk), want, "again")
    rev = pk[::-1].copy()
    same(dedupe(engine, rev), C.reference(rev), "reversed")


def test_feeds_the_keyed_verify(engine, corpus):
    """The golden corpus three times over: dedupe on the device, then cv_ed25519_verify_device_keyed over the result —
    verdicts and status as the corpus records them."""
    reps = 3
    pk = np.tile(corpus["pk"], (reps, 1))
    n = len(pk)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)
    d_pk, d_sig = t(pk, np.uint8), t(np.tile(corpus["sig"], (reps, 1)), np.uint8)
    d_arena = t(np.concatenate([corpus["arena"], np.zeros(16, np.uint8)]), np.uint8)
    d_off, d_len = t(np.tile(corpus["off"], reps), np.uint64), t(np.tile(corpus["len"], reps), np.uint32)
    d_keys = torch.zeros((n, 32), dtype=torch.uint8, device=DEV)
    d_idx = torch.zeros(n, dtype=torch.int32, device=DEV)
    d_nk = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(native.dedupe_keys_workspace(n), dtype=torch.uint8, device=DEV)
    d_bm = torch.zeros((n + 63) // 64, dtype=torch.int64, device=DEV)
    d_st = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    engine.dedupe_keys_device(0, n, d_pk.data_ptr(), d_keys.data_ptr(), d_idx.data_ptr(), d_nk.data_ptr(), ws.data_ptr())
    engine.synchronize(0)
    nk = int(d_nk.cpu()[0])
    want = C.reference(pk)
    assert nk == want[2] and np.array_equal(d_idx.cpu().numpy().view(np.uint32), want[1])
    engine.verify_device_keyed(0, n, nk, d_keys.data_ptr(), d_idx.data_ptr(), d_sig.data_ptr(), d_arena.data_ptr(),
                               d_off.data_ptr(), d_len.data_ptr(), d_bm.data_ptr(), d_st.data_ptr())
    engine.synchronize(0)
    got = native.bitmap_to_bools(d_bm.cpu().numpy().view(np.uint64), n)
    assert np.array_equal(got, np.tile(corpus["verdict"].astype(bool), reps))
    assert np.array_equal(d_st.cpu().numpy(), np.tile(corpus["status"], reps))
