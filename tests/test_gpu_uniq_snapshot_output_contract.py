"""cv_uniq_snapshot's outputs in poisoned, guard-banded buffers (tests/guarded.py) at the header's minimum alignments
(bytes for the keys and ids, 4 for the u32 arrays): a call writes the *n records it reports and nothing else — not the
rest of the arrays, not the guards — at max_entries 1, 63, 64, 65, the resident count and one above it; calls that
report nothing and calls that fail write nothing at all.
"""
import ctypes

import numpy as np
import pytest

import uniq_snapshot_cases as S
from corda_amd import native
from guarded import Guarded

pytestmark = pytest.mark.gpu

RESIDENT = 200
FILLS = (0x00, 0xA5, 0xFF)
DONE = 0xFFFFFFFFFFFFFFFF


def _outputs(m, fill):
    return Guarded([("key", 32 * m, 1), ("id", 32 * m, 1), ("index", 4 * m, 4), ("caller", 4 * m, 4)], fill)


def _call(s, g, cursor, m, n):
    return s._lib.cv_uniq_snapshot(s._h, native._p(cursor), m, g.ptr("key"), g.ptr("id"), g.ptr("index"), g.ptr("caller"),
                                   ctypes.byref(n))


def _used_only(g, m, k, fill, what):
    """The first k records may differ from the fill, the other m - k must not; the guards are whole."""
    g.check_guards(str(what))
    for name, width in (("key", 32), ("id", 32), ("index", 4), ("caller", 4)):
        rest = g.read(name)[width * k:]
        assert (rest == fill).all(), (what, name, "written behind the records used")


@pytest.fixture(scope="module")
def loaded(engine):
    e = S.entries(RESIDENT, 21)
    s = native.UniquenessSet(engine, 256)
    s.load(*e)
    yield s, s.snapshot()
    s.close()


@pytest.mark.parametrize("m", [1, 63, 64, 65, RESIDENT, RESIDENT + 1])
def test_only_the_records_used_are_written(loaded, m):
    s, one = loaded
    for fill in FILLS:
        g = _outputs(m, fill)
        cursor, n, got = np.zeros(2, np.uint64), ctypes.c_size_t(0), [[], [], [], []]
        calls = 0
        while int(cursor[0]) != DONE:
            g.refill()
            what = ("snapshot", m, hex(fill), calls)
            assert _call(s, g, cursor, m, n) == 0, what
            k = n.value
            assert k <= m, what
            _used_only(g, m, k, fill, what)
            got[0].append(g.read("key")[:32 * k].reshape(k, 32))
            got[1].append(g.read("id")[:32 * k].reshape(k, 32))
            got[2].append(g.read("index", np.uint32)[:k])
            got[3].append(g.read("caller", np.uint32)[:k])
            calls += 1
        assert calls == -(-RESIDENT // m) or (m > RESIDENT and calls == 1)
        assert S.same_bytes(tuple(np.concatenate(x) for x in got), one), (m, hex(fill))
        # a finished cursor: CV_OK, nothing written
        g.refill()
        n.value = 5
        assert _call(s, g, cursor, m, n) == 0 and n.value == 0
        _used_only(g, m, 0, fill, ("finished", m, hex(fill)))


def test_calls_that_report_nothing_write_nothing(engine):
    """An empty set, and the windows without an entry of a sparse one."""
    for fill in FILLS:
        g = _outputs(7, fill)
        with native.UniquenessSet(engine, 64) as s:
            cursor, n = np.zeros(2, np.uint64), ctypes.c_size_t(9)
            assert _call(s, g, cursor, 7, n) == 0 and n.value == 0 and int(cursor[0]) == DONE
            _used_only(g, 7, 0, fill, ("empty", hex(fill)))
        with native.UniquenessSet(engine, 1 << 18) as s:
            s.load(*S.entries(5, 5))
            cursor, empty, total = np.zeros(2, np.uint64), 0, 0
            while int(cursor[0]) != DONE:
                g.refill()
                assert _call(s, g, cursor, 7, n) == 0
                _used_only(g, 7, n.value, fill, ("sparse", hex(fill)))
                empty += n.value == 0
                total += n.value
            assert empty >= 1 and total == 5


def test_failed_calls_write_nothing(loaded):
    s, _ = loaded
    for fill in FILLS:
        g = _outputs(7, fill)
        n = ctypes.c_size_t(9)
        cursor = np.zeros(2, np.uint64)
        assert _call(s, g, cursor, 7, n) == 0 and n.value == 7
        stale = np.array([cursor[0], cursor[1] + np.uint64(1)], np.uint64)
        cases = {"stale epoch": (stale, 7), "bad start": (np.array([0, 3], np.uint64), 7),
                 "slot past the table": (np.array([1 << 33, cursor[1]], np.uint64), 7),
                 "no room": (np.zeros(2, np.uint64), 0), "too large": (np.zeros(2, np.uint64), (1 << 30) + 1)}
        for what, (cur, m) in cases.items():
            g.refill()
            n.value = 9
            before = cur.copy()
            rc = _call(s, g, cur, m, n)
            assert rc == (-5 if what == "too large" else -3), (what, rc)
            assert n.value == 9 and np.array_equal(cur, before), what
            _used_only(g, 7, 0, fill, (what, hex(fill)))
        g.refill()
        assert s._lib.cv_uniq_snapshot(s._h, native._p(np.zeros(2, np.uint64)), 7, g.ptr("key"), None, g.ptr("index"),
                                       g.ptr("caller"), ctypes.byref(n)) == -3
        _used_only(g, 7, 0, fill, ("null array", hex(fill)))
