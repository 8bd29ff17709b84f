"""cv_ed25519_verify_device_hotkeys on the GPU (corda_amd/csrc/cv_hotkeys.h, cv_k_hotkeys.hip).  Every
batch is rows of the golden corpus chosen by index, so the expected verdicts and status bytes are the corpus's own
columns (the oracle's), never another route of the engine; the expected split — distinct keys, hot keys, hot and cold
records — is the classification in plain Python (tests/hotkeys_cases.py).  The corpus at three thresholds, the kernel
forms of the sub-batches, the sizes around the wave, CV_BLOCK and CVD_SPAN, the two degenerate decisions, the capacity
rule, the second level of block sums in the record compaction, the output contract in poisoned guard-banded buffers
and repeatability.
"""
import numpy as np
import pytest
import torch

import hotkeys_cases as H
import keydedupe_cases as K
from guarded import DEVICE_ALIGN, Guarded, Options, tail_bits
from corda_amd import native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 0xA7


class Batch:
    """Rows idx of the corpus on the device; the arena is the corpus's, whole."""

    def __init__(self, corpus, idx):
        self.idx = np.asarray(idx)
        self.n = len(self.idx)
        self.pk = np.ascontiguousarray(corpus["pk"][self.idx])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.d_pk, self.d_sig = up(self.pk), up(corpus["sig"][self.idx])
        self.d_arena = up(corpus["arena"])
        self.d_off = up(corpus["off"][self.idx].astype(np.uint64).view(np.int64))
        self.d_len = up(corpus["len"][self.idx].astype(np.uint32).view(np.int32))
        self.ws = torch.full((native.verify_hotkeys_workspace(self.n),), 0x5C, dtype=torch.uint8, device=DEV)
        self.want = corpus["verdict"][self.idx].astype(bool), corpus["status"][self.idx]

    def run(self, engine, hot_min, status=True, fill=POISON):
        """-> (verdicts, status or None, route) through guarded, poisoned outputs at the contract's minimum alignment."""
        n, words = self.n, (self.n + 63) // 64
        g = Guarded([("d_bitmap", 8 * words, DEVICE_ALIGN["d_bitmap"]), ("d_status", n, DEVICE_ALIGN["d_status"])], fill,
                    device=DEV)
        torch.cuda.synchronize()
        route = engine.verify_device_hotkeys(0, n, self.d_pk.data_ptr(), self.d_sig.data_ptr(), self.d_arena.data_ptr(),
                                             self.d_off.data_ptr(), self.d_len.data_ptr(), g.ptr("d_bitmap"),
                                             g.ptr("d_status") if status else 0, self.ws.data_ptr(), hot_min=hot_min)
        engine.synchronize(0)
        g.snapshot()
        g.check_guards(f"n={n} hot_min={hot_min}")              # exactly ceil(n / 64) words, n status bytes, no more
        bm = g.read("d_bitmap", np.uint64)
        assert tail_bits(bm, n) == 0
        if not status:
            assert g.untouched("d_status")
        return native.bitmap_to_bools(bm, n), g.read("d_status") if status else None, route

    def check(self, engine, hot_min, cap=H.CAP, what="", **kw):
        bits, st, route = self.run(engine, hot_min, **kw)
        assert np.array_equal(bits, self.want[0]), (what, np.flatnonzero(bits != self.want[0])[:8])
        if st is not None:
            assert np.array_equal(st, self.want[1]), (what, np.flatnonzero(st != self.want[1])[:8])
        assert (route["nkeys"], route["hot_keys"], route["hot"], route["cold"]) == H.route(self.pk, hot_min, cap), (what, route)
        return route


@pytest.fixture(scope="module")
def own():
    """An engine whose key pool only this module's calls use, kept small (66 KB of tables a key)."""
    e = native.Engine(1)
    e.key_cache_reserve(512)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tiled3(corpus):
    return Batch(corpus, np.tile(np.arange(len(corpus["pk"])), 3))


def moved(engine, before):
    st = engine.key_cache_stats(0)
    return st["hits"] - before["hits"], st["misses"] - before["misses"]


# ---------------------------------------------------------------- 1. the corpus at three thresholds
def test_corpus_splits_at_hot_min_2_and_8(engine, corpus):
    b = Batch(corpus, np.arange(len(corpus["pk"])))
    r2 = b.check(engine, 2, what="x1 hot_min 2")
    assert 0 < r2["hot"] < b.n and (r2["nkeys"], r2["hot_keys"], r2["hot"]) == (324, 76, 451)
    r8 = b.check(engine, 8, what="x1 hot_min 8")
    assert 0 < r8["hot"] < b.n and (r8["hot_keys"], r8["hot"]) == (8, 109)
    assert b.check(engine, 0, what="x1 default") == r8                       # 0 means 8


def test_corpus_tiled_3_makes_the_bad_keys_hot(engine, corpus, tiled3):
    """Every key of the corpus x3 occurs three times or more, the bad keys (once each in the corpus) among them: under
    hot_min 3 and the default capacity the whole batch is hot, under 4 the once-only keys stay cold.  The split of the
    x3 batch under hot_min 3 into both sub-batches is test_bad_keys_hot_beside_cold_records, on a pool of 300 keys."""
    index = K.reference(corpus["pk"])[1]
    bad = corpus["status"] == native.CV_SIG_BAD_KEY
    assert bad.sum() >= 2 and (np.bincount(index)[index[bad]] == 1).all()
    r = tiled3.check(engine, 3, what="x3 hot_min 3")
    assert r["hot"] == tiled3.n and r["hot_keys"] == r["nkeys"]
    r = tiled3.check(engine, 4, what="x3 hot_min 4")
    assert 0 < r["hot"] < tiled3.n


def test_bad_keys_hot_beside_cold_records(corpus):
    """The corpus x3 under hot_min 3 on an engine whose pool holds 300 keys: the first 300 keys in first-seen order are
    hot — bad-key rows among them — and the other 24 cold, so both sub-batches run."""
    e = native.Engine(1)
    try:
        e.key_cache_reserve(300)
        b = Batch(corpus, np.tile(np.arange(len(corpus["pk"])), 3))
        r = b.check(e, 3, cap=300, what="x3 hot_min 3 cap 300")
        assert r["hot_keys"] == 300 and 0 < r["hot"] < b.n
        cls = H.reference(b.pk, 3, 300)[0]
        index = K.reference(b.pk)[1]
        rec_hot = cls[index] != H.COLD
        assert (b.want[1][rec_hot] == native.CV_SIG_BAD_KEY).any()           # a key that is no point, through the keyed path
        assert e.key_cache_stats(0)["capacity"] == 300
    finally:
        e.close()


# ---------------------------------------------------------------- 2. the kernel forms of the sub-batches
@pytest.mark.parametrize("form", ["tri", "quad", "throughput"])
def test_kernel_forms(engine, tiled3, form):
    opts = {"tri": {}, "quad": dict(tri_max=0), "throughput": dict(tri_max=0, quad_max=0)}[form]
    with Options(engine, **opts):
        r = tiled3.check(engine, 4, what=form)
    assert 0 < r["hot"] < tiled3.n


# ---------------------------------------------------------------- 3. size boundaries
def boundary_rows(corpus, n):
    """97 corpus rows drawn often, the others at most once each, a hot record in the last lane."""
    m = len(corpus["pk"])
    rng = np.random.default_rng(n)
    order = rng.permutation(m)
    often, rest = order[:97], order[97:]
    once = rest[:min(len(rest), n // 3)]
    idx = np.concatenate([often[rng.integers(0, 97, n - len(once))], once])
    idx = idx[rng.permutation(n)]
    idx[n - 1] = idx[0] = often[0]
    return idx


@pytest.mark.parametrize("n", (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049))
def test_size_boundaries(engine, corpus, n):
    b = Batch(corpus, boundary_rows(corpus, n))
    r = b.check(engine, 2, what=n)
    assert 0 < r["hot"] < n
    cls, _, perm, nhot = H.reference(b.pk, 2)
    assert perm[n - 1] < nhot                                                # the last lane's record is hot


# ---------------------------------------------------------------- 4. the degenerate decisions
def test_all_cold_leaves_the_key_pool_alone(own, corpus):
    b = Batch(corpus, np.arange(len(corpus["pk"])))
    st = own.key_cache_stats(0)
    r = b.check(own, b.n + 1, cap=512, what="all cold")
    assert r["hot"] == 0 and r["hot_keys"] == 0 and r["cold"] == b.n
    assert own.key_cache_stats(0) == st


def test_all_hot_looks_every_key_up_once(corpus):
    """A pool with room for the batch's 324 keys twice over: key_resolve empties the pool when resident + the call's
    keys pass the capacity, whether or not they are the same keys."""
    e = native.Engine(1)
    try:
        e.key_cache_reserve(1024)
        b = Batch(corpus, np.arange(len(corpus["pk"])))
        st = e.key_cache_stats(0)
        r = b.check(e, 1, cap=1024, what="all hot")
        assert r["hot"] == b.n and r["cold"] == 0 and r["hot_keys"] == r["nkeys"] == 324
        assert moved(e, st) == (0, 324)                                      # one lookup per hot key row, all new
        b.check(e, 1, cap=1024, what="all hot again")
        assert moved(e, st) == (324, 324)
    finally:
        e.close()


# ---------------------------------------------------------------- 5. the capacity rule
def test_candidates_past_the_capacity_are_cold(corpus):
    """cv_key_cache_reserve(4) and eight candidate keys: the first four in first-seen order are hot, the others cold,
    and the pool keeps its capacity."""
    index = K.reference(corpus["pk"])[1]
    once = np.flatnonzero(np.bincount(index)[index] == 1)
    cand, single = once[:8], once[8:40]
    idx = np.concatenate([cand, single[:10], np.repeat(cand[::-1], 2), single[10:]])
    e = native.Engine(1)
    try:
        e.key_cache_reserve(4)
        b = Batch(corpus, idx)
        st = e.key_cache_stats(0)
        r = b.check(e, 2, cap=4, what="capacity 4")
        assert (r["nkeys"], r["hot_keys"], r["hot"], r["cold"]) == (40, 4, 12, b.n - 12)
        cls = H.reference(b.pk, 2, 4)[0]
        assert cls[:8].tolist() == [0, 1, 2, 3] + [H.COLD] * 4               # first-seen, not by count or by luck
        after = e.key_cache_stats(0)
        assert after["capacity"] == 4 and after["misses"] - st["misses"] == 4 and after["resident"] == 4
    finally:
        e.close()


# ---------------------------------------------------------------- 6. the second level of block sums
def test_second_level_of_block_sums(engine, corpus):
    """n = 1024 * 1024 + 1: the smallest batch whose record compaction takes a second level of block sums.  Eight
    corpus rows hot, the last record the only occurrence of its key."""
    n = 1024 * 1024 + 1
    index = K.reference(corpus["pk"])[1]
    once = np.flatnonzero(np.bincount(index)[index] == 1)
    hot_rows, last = once[:8], once[8]
    others = np.setdiff1d(np.arange(len(index)), once[:9])
    rng = np.random.default_rng(6)
    idx = np.where(rng.integers(0, 4, n) != 0, hot_rows[rng.integers(0, 8, n)], others[rng.integers(0, len(others), n)])
    idx[n - 1] = last
    b = Batch(corpus, idx)
    r = b.check(engine, 50000, what="2^20 + 1")
    assert r["hot_keys"] == 8 and 0 < r["hot"] < n and r["cold"] > 1024
    assert H.reference(b.pk, 50000)[2][n - 1] == n - 1                       # cold, and the last row of the cold sub-batch


# ---------------------------------------------------------------- 7. the output contract
@pytest.mark.parametrize("n", (65, 699))
def test_output_contract(engine, corpus, n):
    b = Batch(corpus, boundary_rows(corpus, n) if n != len(corpus["pk"]) else np.arange(n))
    for fill in (0xA7, 0x00, 0xFF):                                          # nothing is ORed in, nothing left alone
        r = b.check(engine, 2, what=(n, fill), fill=fill)
        assert 0 < r["hot"] < n
    b.check(engine, 2, what=(n, "no status"), status=False)                  # d_status = NULL is accepted
    b.check(engine, n + 1, what=(n, "all cold, no status"), status=False)


# ---------------------------------------------------------------- 8. repeatability
def test_repeatable_and_order_follows_the_input(engine, corpus):
    m = len(corpus["pk"])
    b = Batch(corpus, np.arange(m))
    first = b.run(engine, 2)
    second = b.run(engine, 2)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1]) and first[2] == second[2]
    rev = Batch(corpus, np.arange(m)[::-1].copy())
    r = rev.check(engine, 2, what="reversed")
    assert (r["nkeys"], r["hot_keys"], r["hot"]) == (first[2]["nkeys"], first[2]["hot_keys"], first[2]["hot"])
