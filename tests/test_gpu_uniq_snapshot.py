"""Snapshot, clear and install of the uniqueness set on the GPU (cv_uniq_snapshot / cv_uniq_clear / cv_uniq_install: the
kernels of corda_amd/csrc/cv_k_uniq.hip through the C-ABI and native.UniquenessSet) against the dict model of
tests/uniq_snapshot_cases.py, the literal DistributedImmutableMap (DistributedImmutableMap.kt:59-105).

The seams of the count / scan / emit: a block of the kernels covers 256 slots, so every table here (16 slots at the
least, one wave's worth) but the smallest spans several blocks; the shared scan of the block totals takes one block up
to 1,024 totals = 262,144 slots of a call's window and a second level above that.  The large set (150,000 entries in
524,288 slots) is read with windows of 300,000 slots (1,172 block totals: the second level) and of 65,536 slots (256
totals: one block).
"""
import ctypes

import numpy as np
import pytest

import uniq_cases as C
import uniq_snapshot_cases as S
from corda_amd import native

pytestmark = pytest.mark.gpu

NAMES = ("tx_status", "state_conflict", "cons_id", "cons_index", "cons_caller")
DONE = 0xFFFFFFFFFFFFFFFF
ABSENT = C.keys_array([C.key_of("absent", i) for i in range(40)])


def _commit(s, batch):
    f = C.flatten(batch)
    return dict(zip(NAMES, s.commit_batch(f["key"], f["begin"], f["id"], f["caller"], f["enable"])))


def _call(s, cursor, m, bufs, n):
    return s._lib.cv_uniq_snapshot(s._h, native._p(cursor), m, *[native._p(b) for b in bufs], ctypes.byref(n))


def _bufs(m, fill=0):
    return (np.full((m, 32), fill, np.uint8), np.full((m, 32), fill, np.uint8), np.full(m, fill, np.uint32),
            np.full(m, fill, np.uint32))


def test_empty_and_one_entry(engine):
    with native.UniquenessSet(engine, 100) as s:
        S.check_passes(s, {}, what="empty")
        cursor, n, bufs = np.zeros(2, np.uint64), ctypes.c_size_t(9), _bufs(3, 7)
        assert _call(s, cursor, 3, bufs, n) == 0 and n.value == 0 and int(cursor[0]) == DONE
        n.value = 9
        assert _call(s, cursor, 3, bufs, n) == 0 and n.value == 0          # a finished cursor yields nothing
        assert all((b == 7).all() for b in bufs)
        e = S.entries(1, 1)
        s.load(*e)
        S.check_passes(s, S.model_of(e), what="one")


def test_full_small_table_and_growth(engine):
    """16 slots filled to the capacity of 8 (the seed is the set's own, so whether a probe wraps is its business: the
    CPU harness pins that case), then growth to 2,048 slots and 400 more entries."""
    batch, e = S.wrap_entries()
    more = S.entries(400, 2)
    with native.UniquenessSet(engine, 8) as s:
        assert (_commit(s, batch)["tx_status"] == C.OK).all()
        st = s.stats()
        assert (st["slots"], st["resident"]) == (16, 8)
        S.check_passes(s, S.model_of(e), chunks=(1, 7, 8, 9), what="full")
        s.reserve(1024)
        s.load(*more)
        S.check_passes(s, S.model_of(e, more), what="growth")


def test_three_thousand_entries_in_8192_slots(engine):
    e = S.entries(3000, 3)
    with native.UniquenessSet(engine, 4096) as s:
        s.load(*e)
        assert s.stats()["slots"] == 8192
        S.check_passes(s, S.model_of(e), what="3000")


def test_one_record_a_call(engine):
    e = S.entries(300, 4)
    with native.UniquenessSet(engine, 300) as s:
        s.load(*e)
        one = s.snapshot()
        parts = list(s.snapshot_chunks(1))
        assert len(parts) == 300 and all(len(p[2]) == 1 for p in parts)
        assert S.same_bytes(tuple(np.concatenate([p[j] for p in parts]) for j in range(4)), one)


def test_windows_of_empty_slots(engine):
    """2^19 slots and five entries: eight calls of 65,536 slots, some of which report nothing without being the last."""
    e = S.entries(5, 5)
    with native.UniquenessSet(engine, 1 << 18) as s:
        s.load(*e)
        assert s.stats()["slots"] == 1 << 19
        parts = list(s.snapshot_chunks(7))
        assert len(parts) == 8 and any(len(p[2]) == 0 for p in parts[:-1])
        assert S.as_model(tuple(np.concatenate([p[j] for p in parts]) for j in range(4))) == S.model_of(e)


def test_large_set_crosses_the_scan_levels(engine):
    """150,000 entries in 524,288 slots (the module docstring names the seams): the whole pass takes two calls of
    300,000 slots, each scanned at two levels; the chunked passes use 65,536-slot windows (one level) and, at 40,000
    records a call, 80,000-slot windows that end by the record count in mid-window."""
    e = S.entries(150000, 6)
    with native.UniquenessSet(engine, 1 << 18) as s:
        s.load(*e)
        assert s.stats()["slots"] == 1 << 19
        S.check_passes(s, S.model_of(e), chunks=(1000, 40000), what="large")


def test_device_to_device(engine):
    """Snapshot of A installed into B, opened separately (another seed) with a smaller capacity over other contents:
    the same resident count, lookups and snapshot as a set, and the same follow-up commit, with the serial tail alone
    on B and the default rounds on A, gives identical arrays."""
    e = S.entries(3000, 3)
    model = S.model_of(e)
    old = S.entries(50, 8)
    with native.UniquenessSet(engine, 4096) as a, native.UniquenessSet(engine, 64) as b:
        a.load(*e)
        b.load(*old)
        b.set_max_rounds(0)
        b.install(*a.snapshot())
        sa, sb = a.stats(), b.stats()
        assert sb["resident"] == sa["resident"] == 3000 and (sb["capacity"], sb["slots"]) == (3000, 8192)
        S.check_lookups(b, model, np.concatenate([ABSENT, old[0]]))
        for x, y in zip(a.lookup(np.concatenate([e[0], ABSENT])), b.lookup(np.concatenate([e[0], ABSENT]))):
            assert np.array_equal(x, y)
        assert S.as_model(b.snapshot()) == model
        batch = S.follow_up([k.tobytes() for k in e[0][:500]])
        a.reserve(8192)
        b.reserve(8192)
        fa, fb = _commit(a, batch), _commit(b, batch)
        C.assert_same(fa, fb, "follow-up")
        assert 0 < int((fa["tx_status"] == C.CONFLICT).sum()) < len(batch)
        assert b.stats()["rounds"] == 0 and a.stats()["rounds"] >= 1
        assert S.as_model(a.snapshot()) == S.as_model(b.snapshot())
        b.install(*S.entries(3, 9))                                        # the capacity never shrinks
        assert b.stats()["capacity"] == 8192 and b.stats()["resident"] == 3
        b.install(*S.entries(0, 9))                                        # n == 0 is clear
        assert b.stats()["resident"] == 0 and len(b.snapshot()[2]) == 0


def test_failed_install_leaves_the_set_as_it_was(engine):
    """A repeated key (CV_E_ARGS) and n above 2^30 (CV_E_TOO_LARGE): byte-identical under snapshot, the same
    statistics.  (The third failure, no memory for the second table, cannot be had at a test's sizes.)"""
    e = S.entries(200, 10)
    with native.UniquenessSet(engine, 256) as s:
        s.load(*e)
        before, st = s.snapshot(), s.stats()
        bad = S.entries(500, 11)
        bad[0][499] = bad[0][17]
        with pytest.raises(native.CvError) as ei:
            s.install(*bad)
        assert ei.value.code == -3
        p = native._p
        assert s._lib.cv_uniq_install(s._h, (1 << 30) + 1, p(bad[0]), p(bad[1]), p(bad[2]), p(bad[3])) == -5
        assert S.same_bytes(s.snapshot(), before) and s.stats() == st
        S.check_lookups(s, S.model_of(e), bad[0][:100])


def test_clear_then_recommit(engine):
    batch, e = S.wrap_entries()
    with native.UniquenessSet(engine, 16) as s:
        assert (_commit(s, batch)["tx_status"] == C.OK).all()
        assert (_commit(s, batch)["tx_status"] == C.CONFLICT).all()
        s.clear()
        st = s.stats()
        assert (st["resident"], st["capacity"], st["slots"]) == (0, 16, 32)
        S.check_lookups(s, {}, e[0])
        assert len(s.snapshot()[2]) == 0
        assert (_commit(s, batch)["tx_status"] == C.OK).all()
        assert S.as_model(s.snapshot()) == S.model_of(e)


def _notarise_one(engine, s):
    """One non-validating cv_notarise_batch on the set: one transaction of two leaves, the first its input state."""
    arena = np.frombuffer(b"an input state of the epoch test" + b"an output", np.uint8).copy()
    off, ln, begin = np.array([0, 32], np.uint64), np.array([32, 9], np.uint32), np.array([0, 2], np.uint32)
    ids, st = engine.merkle_tx_ids(arena, off, ln, begin)
    assert st[0] == 0
    signer = native.Signer(engine, bytes(range(32)))
    try:
        out = engine.notarise_batch(s, signer, arena, off, ln, begin, np.array([1], np.uint32), ids, np.array([3], np.uint32))
        assert out["outcome"][0] == native.CV_NS_SUCCESS
    finally:
        signer.close()


def test_a_notarise_batch_between_two_chunks_ends_the_pass(engine):
    e = S.entries(300, 6)
    with native.UniquenessSet(engine, 600) as s:
        s.load(*e)
        cursor, n, bufs = np.zeros(2, np.uint64), ctypes.c_size_t(0), _bufs(7)
        assert _call(s, cursor, 7, bufs, n) == 0 and n.value == 7
        _notarise_one(engine, s)
        assert s.stats()["resident"] == 301
        for b in bufs:
            b[...] = 0xEE
        assert _call(s, cursor, 7, bufs, n) == -3 and n.value == 7 and all((b == 0xEE).all() for b in bufs)
        assert len(S.as_model(s.snapshot())) == 301


@pytest.mark.parametrize("what", ["commit", "load", "clear", "install", "reserve"])
def test_epoch_refuses_a_continued_pass(engine, what):
    e = S.entries(300, 6)
    more = S.entries(10, 77)
    with native.UniquenessSet(engine, 600) as s:
        s.load(*e)
        cursor, n, bufs = np.zeros(2, np.uint64), ctypes.c_size_t(0), _bufs(7)
        assert _call(s, cursor, 7, bufs, n) == 0 and n.value == 7
        s.lookup(e[0][:5])                          # what changes nothing leaves the pass alone
        s.stats()
        s.reserve(601)                              # the slots already hold it: no rehash
        list(s.snapshot_chunks(100))
        assert _call(s, cursor, 7, bufs, n) == 0 and n.value == 7
        {"commit": lambda: _commit(s, [([C.key_of("ep", 0)], C.tx_id_of("ep", 0), 1, True)]),
         "load": lambda: s.load(*more), "clear": s.clear, "install": lambda: s.install(*e),
         "reserve": lambda: s.reserve(5000)}[what]()
        before = cursor.copy()
        for b in bufs:
            b[...] = 0xEE
        n.value = 99
        assert _call(s, cursor, 7, bufs, n) == -3
        assert np.array_equal(cursor, before) and n.value == 99 and all((b == 0xEE).all() for b in bufs)
        assert _call(s, np.array([0, 5], np.uint64), 7, bufs, n) == -3
        assert _call(s, np.array([1 << 40, before[1]], np.uint64), 7, bufs, n) == -3
        with native.UniquenessSet(engine, 600) as t:                       # a cursor of another set
            t.load(*e)
            assert _call(t, cursor.copy(), 7, bufs, n) == -3
        S.as_model(s.snapshot())
