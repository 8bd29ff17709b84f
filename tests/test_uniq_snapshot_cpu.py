"""Snapshot, clear and install of the uniqueness set compiled for the CPU (the per-lane pieces of
corda_amd/csrc/cv_uniq.h through tests/uniq_snapshot_harness.cpp) against a dict model, the literal
DistributedImmutableMap (DistributedImmutableMap.kt:59-105): the cases of tests/uniq_snapshot_cases.py with the lanes
of every step in ascending, descending and one shuffled order; the cursor, the epoch that refuses a torn pass; install
into a set with another seed and capacity; the C-ABI's argument checks that need no device; and the same core under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program (tests/uniq_snapshot_san.cpp).  No GPU.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import uniq_cases as C
import uniq_snapshot_cases as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
ORDERS = (0, 1, 2)
DONE = 0xFFFFFFFFFFFFFFFF
HARNESS = [os.path.join(REPO, "tests", "uniq_snapshot_harness.cpp"), os.path.join(REPO, "tests", "uniq_harness.cpp"),
           os.path.join(REPO, "corda_amd", "csrc", "cv_uniq.h"), os.path.join(REPO, "corda_amd", "csrc", "cv_table.h")]


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def harness():
    """tests/uniq_snapshot_harness.cpp built as tests/test_uniq_cpu.py builds its harness."""
    lib = os.path.join(REPO, "tests", "_build", "libcvuniqsnap.so")
    if _stale(lib, HARNESS):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-O2", "-std=c++17", "-fPIC",
                        "-shared", HARNESS[0], "-o", lib], check=True)
    h = ctypes.CDLL(lib)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    h.hus_open.restype = vp
    h.hus_open.argtypes = [u64, u64, u64]
    h.hus_close.argtypes = [vp]
    h.hus_set.restype = vp
    h.hus_set.argtypes = [vp]
    h.huq_stats.argtypes = [vp, vp]
    h.huq_lookup.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_int] + [vp] * 4
    h.hus_commit.argtypes = [vp, ctypes.c_uint32] + [vp] * 5 + [ctypes.c_int] * 2 + [vp] * 5
    h.hus_load.argtypes = [vp, ctypes.c_uint32] + [vp] * 4 + [ctypes.c_int]
    h.hus_reserve.argtypes = [vp, u64, ctypes.c_int]
    h.hus_snapshot.argtypes = [vp, vp, u64, ctypes.c_int] + [vp] * 5
    h.hus_clear.argtypes = [vp]
    h.hus_install.argtypes = [vp, u64] + [vp] * 4 + [u64, ctypes.c_int]
    return h


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class HostSet:
    """One set of the harness with the calls of native.UniquenessSet."""

    def __init__(self, h, capacity, seed=0x243F6A8885A308D3, order=0, max_rounds=8, epoch=1):
        self.h, self.order, self.max_rounds = h, order, max_rounds
        self.p = h.hus_open(capacity, seed, epoch)

    def close(self):
        self.h.hus_close(self.p)

    def stats(self):
        out = np.zeros(7, np.uint64)
        self.h.huq_stats(self.h.hus_set(self.p), _p(out))
        return dict(zip(("resident", "capacity", "slots", "rounds", "tail", "probe", "wraps"), map(int, out)))

    def commit(self, f):
        n = max(f["nstates"], 1)
        out = dict(tx_status=np.zeros(f["ntx"], np.uint8), state_conflict=np.zeros(n, np.uint8),
                   cons_id=np.zeros((n, 32), np.uint8), cons_index=np.zeros(n, np.uint32), cons_caller=np.zeros(n, np.uint32))
        key = f["key"] if f["nstates"] else np.zeros((1, 32), np.uint8)
        assert self.h.hus_commit(self.p, f["ntx"], _p(key), _p(f["begin"]), _p(f["id"]), _p(f["caller"]), _p(f["enable"]),
                                 self.max_rounds, self.order, *[_p(out[k]) for k in
                                                                ("tx_status", "state_conflict", "cons_id", "cons_index",
                                                                 "cons_caller")]) == 0
        for k in ("state_conflict", "cons_id", "cons_index", "cons_caller"):
            out[k] = out[k][:f["nstates"]]
        return out

    def lookup(self, keys):
        n = len(keys)
        m = max(n, 1)
        found, cid = np.zeros(m, np.uint8), np.zeros((m, 32), np.uint8)
        cix, cc = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        assert self.h.huq_lookup(self.h.hus_set(self.p), n, _p(np.ascontiguousarray(keys)), self.order, _p(found), _p(cid),
                                 _p(cix), _p(cc)) == 0
        return found[:n], cid[:n], cix[:n], cc[:n]

    def load(self, key, cid, cix, cc):
        return self.h.hus_load(self.p, len(key), _p(key), _p(cid), _p(cix.copy()), _p(cc), self.order)

    def reserve(self, capacity):
        return self.h.hus_reserve(self.p, capacity, self.order)

    def clear(self):
        return self.h.hus_clear(self.p)

    def install(self, key, cid, cix, cc, seed=0x9E3779B97F4A7C15):
        return self.h.hus_install(self.p, len(key), _p(np.ascontiguousarray(key)), _p(np.ascontiguousarray(cid)),
                                  _p(cix.copy()), _p(np.ascontiguousarray(cc)), seed, self.order)

    def snapshot_call(self, cursor, m, bufs, n):
        return self.h.hus_snapshot(self.p, _p(cursor), m, self.order, *[_p(b) for b in bufs], _p(n))

    def snapshot_chunks(self, m):
        cursor = np.zeros(2, np.uint64)
        bufs = (np.zeros((m, 32), np.uint8), np.zeros((m, 32), np.uint8), np.zeros(m, np.uint32), np.zeros(m, np.uint32))
        n = np.zeros(1, np.uint64)
        while int(cursor[0]) != DONE:
            assert self.snapshot_call(cursor, m, bufs, n) == 0
            yield tuple(b[:int(n[0])].copy() for b in bufs)

    def snapshot(self, max_entries=None):
        m = max(self.stats()["resident"], 1) if max_entries is None else max_entries
        parts = list(self.snapshot_chunks(m))
        return tuple(np.concatenate([p[j] for p in parts]) for j in range(4))


ABSENT = C.keys_array([C.key_of("absent", i) for i in range(40)])


@pytest.mark.parametrize("order", ORDERS)
def test_empty_and_one_entry(harness, order):
    s = HostSet(harness, 100, order=order)
    S.check_passes(s, {}, what="empty")
    cursor, n = np.zeros(2, np.uint64), np.full(1, 9, np.uint64)
    bufs = (np.full((3, 32), 7, np.uint8), np.full((3, 32), 7, np.uint8), np.full(3, 7, np.uint32), np.full(3, 7, np.uint32))
    assert s.snapshot_call(cursor, 3, bufs, n) == 0 and n[0] == 0 and int(cursor[0]) == DONE
    n[0] = 9
    assert s.snapshot_call(cursor, 3, bufs, n) == 0 and n[0] == 0          # a finished cursor yields nothing
    assert all((b == 7).all() for b in bufs)
    e = S.entries(1, 1)
    assert s.load(*e) == 0
    S.check_passes(s, S.model_of(e), what="one")
    s.close()


@pytest.mark.parametrize("order", ORDERS)
def test_full_small_table_whose_probes_wrap(harness, order):
    """16 slots filled to the capacity of 8; a probe passed the last slot, so an entry's slot lies before its hash's."""
    batch, e = S.wrap_entries()
    s = HostSet(harness, 8, seed=S.WRAP_SEED, order=order)
    s.commit(C.flatten(batch))
    st = s.stats()
    assert (st["slots"], st["resident"]) == (16, 8) and st["wraps"] >= 1
    S.check_passes(s, S.model_of(e), chunks=(1, 7, 8, 9), what="wrap")
    s.close()


@pytest.mark.parametrize("order", ORDERS)
def test_after_growth(harness, order):
    batch, e = S.wrap_entries()
    more = S.entries(400, 2)
    s = HostSet(harness, 8, seed=S.WRAP_SEED, order=order)
    s.commit(C.flatten(batch))
    assert s.reserve(1024) == 0 and s.load(*more) == 0
    S.check_passes(s, S.model_of(e, more), what="growth")
    s.close()


@pytest.mark.parametrize("order", ORDERS)
def test_three_thousand_entries_in_8192_slots(harness, order):
    e = S.entries(3000, 3)
    s = HostSet(harness, 4096, order=order)
    assert s.load(*e) == 0 and s.stats()["slots"] == 8192
    one = S.check_passes(s, S.model_of(e), what="3000")
    if order == 0:
        # the records do not depend on the lane order: the other orders give these very bytes
        for o in ORDERS[1:]:
            t = HostSet(harness, 4096, order=o)
            assert t.load(*e) == 0                 # inserted in another order: other slots, so compare as a set only
            assert S.as_model(t.snapshot()) == S.as_model(one)
            s.order = o
            assert S.same_bytes(s.snapshot(), one)
            t.close()
    s.close()


def test_one_record_a_call(harness):
    e = S.entries(300, 4)
    s = HostSet(harness, 300)
    assert s.load(*e) == 0
    one = s.snapshot()
    parts = list(s.snapshot_chunks(1))
    assert len(parts) == 300 and all(len(p[2]) == 1 for p in parts)
    assert S.same_bytes(tuple(np.concatenate([p[j] for p in parts]) for j in range(4)), one)
    s.close()


@pytest.mark.parametrize("order", ORDERS)
def test_windows_of_empty_slots(harness, order):
    """2^19 slots and five entries: a call looks at 65,536 slots, so the pass takes eight calls and some of them report
    nothing without being the last — a caller loops on the cursor."""
    e = S.entries(5, 5)
    s = HostSet(harness, 1 << 18, order=order)
    assert s.load(*e) == 0 and s.stats()["slots"] == 1 << 19
    parts = list(s.snapshot_chunks(7))
    assert len(parts) == 8 and any(len(p[2]) == 0 for p in parts[:-1])
    assert S.as_model(tuple(np.concatenate([p[j] for p in parts]) for j in range(4))) == S.model_of(e)
    s.close()


def _mutations(e):
    batch = [([C.key_of("ep", 0)], C.tx_id_of("ep", 0), 1, True)]
    more = S.entries(10, 77)
    return {"commit": lambda s: s.commit(C.flatten(batch)),
            "load": lambda s: s.load(*more),
            "clear": lambda s: s.clear(),
            "install": lambda s: s.install(*e),
            "reserve": lambda s: s.reserve(5000)}


@pytest.mark.parametrize("what", ["commit", "load", "clear", "install", "reserve"])
def test_epoch_refuses_a_continued_pass(harness, what):
    e = S.entries(300, 6)
    s = HostSet(harness, 600, epoch=0x1234)
    assert s.load(*e) == 0
    cursor, n = np.zeros(2, np.uint64), np.zeros(1, np.uint64)
    bufs = (np.zeros((7, 32), np.uint8), np.zeros((7, 32), np.uint8), np.zeros(7, np.uint32), np.zeros(7, np.uint32))
    assert s.snapshot_call(cursor, 7, bufs, n) == 0 and n[0] == 7
    # what changes nothing leaves the pass alone
    s.lookup(e[0][:5])
    s.stats()
    assert s.reserve(601) == 0                      # the slots already hold it: no rehash
    list(s.snapshot_chunks(100))
    assert s.snapshot_call(cursor, 7, bufs, n) == 0 and n[0] == 7
    _mutations(e)[what](s)
    before = cursor.copy()
    for b in bufs:
        b[...] = 0xEE
    n[0] = 99
    assert s.snapshot_call(cursor, 7, bufs, n) == -3
    assert np.array_equal(cursor, before) and n[0] == 99 and all((b == 0xEE).all() for b in bufs)
    # a cursor no pass gave: a start with a stale epoch word, a slot past the table
    assert s.snapshot_call(np.array([0, 5], np.uint64), 7, bufs, n) == -3
    assert s.snapshot_call(np.array([1 << 40, before[1]], np.uint64), 7, bufs, n) == -3
    # a fresh pass works
    S.as_model(s.snapshot())
    s.close()


@pytest.mark.parametrize("order", ORDERS)
def test_install_into_another_seed_and_capacity(harness, order):
    e = S.entries(3000, 3)
    model = S.model_of(e)
    a = HostSet(harness, 4096, order=order)
    assert a.load(*e) == 0
    snap = a.snapshot()
    b = HostSet(harness, 64, seed=0x1111, order=order, max_rounds=0)
    old = S.entries(50, 8)
    assert b.load(*old) == 0                       # install replaces what the set held
    assert b.install(*snap, seed=0x2222) == 0
    st = b.stats()
    assert (st["resident"], st["capacity"], st["slots"]) == (3000, 3000, 8192)
    S.check_lookups(b, model, np.concatenate([ABSENT, old[0]]))
    assert S.as_model(b.snapshot()) == model
    batch = S.follow_up([k.tobytes() for k in e[0][:500]])
    assert a.reserve(8192) == 0 and b.reserve(8192) == 0
    fa, fb = a.commit(C.flatten(batch)), b.commit(C.flatten(batch))
    C.assert_same(fa, fb, "follow-up")
    assert 0 < int((fa["tx_status"] == C.CONFLICT).sum()) < len(batch)
    assert S.as_model(a.snapshot()) == S.as_model(b.snapshot())
    # the capacity never shrinks
    assert b.install(*S.entries(3, 9)) == 0 and b.stats()["capacity"] == 8192 and b.stats()["resident"] == 3
    assert b.install(*S.entries(0, 9)) == 0 and b.stats()["resident"] == 0
    a.close()
    b.close()


def test_install_with_a_repeated_key_changes_nothing(harness):
    e = S.entries(200, 10)
    s = HostSet(harness, 256)
    assert s.load(*e) == 0
    before, st = s.snapshot(), s.stats()
    bad = S.entries(500, 11)
    bad[0][499] = bad[0][17]
    assert s.install(*bad) == -3
    assert harness.hus_install(s.p, (1 << 30) + 1, _p(bad[0]), _p(bad[1]), _p(bad[2]), _p(bad[3]), 1, 0) == -5
    assert S.same_bytes(s.snapshot(), before) and s.stats() == st
    s.close()


def test_clear_then_recommit(harness):
    batch, e = S.wrap_entries()
    s = HostSet(harness, 16)
    assert (s.commit(C.flatten(batch))["tx_status"] == C.OK).all()
    assert (s.commit(C.flatten(batch))["tx_status"] == C.CONFLICT).all()
    assert s.clear() == 0
    st = s.stats()
    assert (st["resident"], st["capacity"], st["slots"]) == (0, 16, 32)
    S.check_lookups(s, {}, e[0])
    assert len(s.snapshot()[2]) == 0
    assert (s.commit(C.flatten(batch))["tx_status"] == C.OK).all()
    assert S.as_model(s.snapshot()) == S.model_of(e)
    s.close()


def test_argument_checks_without_a_device():
    """The checks of the three calls that run before any device call; a failed call writes nothing."""
    from corda_amd import native
    lib = native.load()
    ARGS, TOO_LARGE = -3, -5
    cur = np.zeros(2, np.uint64)
    key, cid = np.full((4, 32), 9, np.uint8), np.full((4, 32), 9, np.uint8)
    cix, cc = np.full(4, 9, np.uint32), np.full(4, 9, np.uint32)
    n = ctypes.c_size_t(77)
    h = ctypes.c_void_p(1)                          # never dereferenced: every call below fails before the set is read

    def snap(u=h, cursor=cur, m=4, k=key, i=cid, x=cix, c=cc, nn=ctypes.byref(n)):
        return lib.cv_uniq_snapshot(u, _p(cursor), m, _p(k), _p(i), _p(x), _p(c), nn)

    assert snap(m=0) == ARGS
    assert snap(cursor=None) == ARGS and snap(nn=None) == ARGS
    assert snap(k=None) == ARGS and snap(i=None) == ARGS and snap(x=None) == ARGS and snap(c=None) == ARGS
    assert snap(m=(1 << 30) + 1) == TOO_LARGE
    assert snap(u=None) == ARGS
    assert lib.cv_uniq_clear(None) == ARGS
    assert lib.cv_uniq_install(None, 0, None, None, None, None) == ARGS          # n == 0 is clear: the null set
    assert lib.cv_uniq_install(h, 4, None, _p(cid), _p(cix), _p(cc)) == ARGS
    assert lib.cv_uniq_install(h, 4, _p(key), None, _p(cix), _p(cc)) == ARGS
    assert lib.cv_uniq_install(h, 4, _p(key), _p(cid), None, _p(cc)) == ARGS
    assert lib.cv_uniq_install(h, 4, _p(key), _p(cid), _p(cix), None) == ARGS
    assert lib.cv_uniq_install(h, (1 << 30) + 1, _p(key), _p(cid), _p(cix), _p(cc)) == TOO_LARGE
    assert lib.cv_uniq_install(None, 4, _p(key), _p(cid), _p(cix), _p(cc)) == ARGS
    assert n.value == 77 and not cur.any() and (key == 9).all() and (cid == 9).all() and (cix == 9).all() and (cc == 9).all()
    for name in ("cv_uniq_snapshot", "cv_uniq_clear", "cv_uniq_install"):
        assert name in native.EXPORTED


def test_sanitizers_standalone_program():
    """tests/uniq_snapshot_san.cpp (its own main: the wrap, chunk-seam and install cases against a std::map) under
    ASan + UBSan, run as a child process: nothing is loaded into this process under a sanitizer."""
    exe = os.path.join(REPO, "tests", "_build", "uniq_snapshot_san")
    src = os.path.join(REPO, "tests", "uniq_snapshot_san.cpp")
    if _stale(exe, [src] + HARNESS):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-O1", "-g", "-std=c++17",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                        "-Xarch_host", "-fno-omit-frame-pointer", src, "-o", exe, "-fsanitize=address,undefined"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    for bad in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"):
        assert bad not in out, out[-4000:]
    assert r.stdout.split()[0] == "ok"
