"""The uniqueness set's core compiled for the CPU (corda_amd/csrc/cv_uniq.h through tests/uniq_harness.cpp) against
InMemoryUniquenessProvider, exactly: the cases of tests/uniq_cases.py with the lanes of every step run in ascending,
descending and one shuffled order and with max_rounds 0, 1 and the default; the probe that wraps past the table's
end; growth; load; the C-ABI's argument checks that need no device; and the same core under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/uniq_san.cpp).  No GPU.

Reference: UniquenessProvider.kt:13-35, InMemoryUniquenessProvider.kt:14-36, UniquenessProviderTests.kt.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import uniq_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
DEFAULT_ROUNDS = 8
ORDERS = (0, 1, 2)              # the harness's lane orders: ascending, descending, shuffled


def _deps(*srcs):
    return list(srcs) + [os.path.join(REPO, "corda_amd", "csrc", h) for h in ("cv_uniq.h", "cv_table.h")]


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def harness():
    """tests/uniq_harness.cpp built as tests/test_pmt_build.py builds its harness."""
    lib = os.path.join(REPO, "tests", "_build", "libcvuniq.so")
    src = os.path.join(REPO, "tests", "uniq_harness.cpp")
    if _stale(lib, _deps(src)):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-O2", "-std=c++17", "-fPIC",
                        "-shared", src, "-o", lib], check=True)
    h = ctypes.CDLL(lib)
    h.huq_open.restype = ctypes.c_void_p
    h.huq_open.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    h.huq_close.argtypes = [ctypes.c_void_p]
    h.huq_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    h.huq_reserve.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]
    h.huq_commit.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 5
    h.huq_lookup.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    h.huq_load.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4 + [ctypes.c_int]
    return h


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class HostSet:
    """One set of the harness with the calls of native.UniquenessSet."""

    def __init__(self, h, capacity, seed=0x243F6A8885A308D3, order=0, max_rounds=DEFAULT_ROUNDS):
        self.h, self.order, self.max_rounds = h, order, max_rounds
        self.p = h.huq_open(capacity, seed)

    def close(self):
        self.h.huq_close(self.p)

    def stats(self):
        out = np.zeros(7, np.uint64)
        self.h.huq_stats(self.p, _p(out))
        return dict(zip(("resident", "capacity", "slots", "rounds", "tail", "probe", "wraps"), map(int, out)))

    def commit_rc(self, f, fill=0):
        S = max(f["nstates"], 1)
        out = dict(tx_status=np.full(f["ntx"], fill, np.uint8), state_conflict=np.full(S, fill, np.uint8),
                   cons_id=np.full((S, 32), fill, np.uint8), cons_index=np.full(S, fill, np.uint32),
                   cons_caller=np.full(S, fill, np.uint32))
        key = f["key"] if f["nstates"] else np.zeros((1, 32), np.uint8)
        rc = self.h.huq_commit(self.p, f["ntx"], _p(key), _p(f["begin"]), _p(f["id"]), _p(f["caller"]), _p(f["enable"]),
                               self.max_rounds, self.order, *[_p(out[k]) for k in
                                                              ("tx_status", "state_conflict", "cons_id", "cons_index", "cons_caller")])
        for k in ("state_conflict", "cons_id", "cons_index", "cons_caller"):
            out[k] = out[k][:f["nstates"]]
        return rc, out

    def commit(self, f):
        rc, out = self.commit_rc(f)
        assert rc == 0
        return out

    def lookup(self, keys):
        n = len(keys)
        found, cid = np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
        cix, cc = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        assert self.h.huq_lookup(self.p, n, _p(keys), self.order, _p(found), _p(cid), _p(cix), _p(cc)) == 0
        return found, cid, cix, cc

    def load(self, keys, ids, index, caller):
        return self.h.huq_load(self.p, len(keys), _p(keys), _p(ids), _p(np.ascontiguousarray(index, np.uint32)),
                               _p(np.ascontiguousarray(caller, np.uint32)), self.order)

    def reserve(self, capacity):
        return self.h.huq_reserve(self.p, capacity, self.order)


@pytest.fixture(scope="module")
def cases():
    return {name: make() for name, make in C.CASES.items()}


@pytest.mark.parametrize("max_rounds", [0, 1, DEFAULT_ROUNDS])
@pytest.mark.parametrize("name", list(C.CASES))
def test_cases_in_every_lane_order(harness, cases, name, max_rounds):
    """(a)-(f) against the oracle: statuses, every conflict's state -> (id, index, caller), and the lookup of every
    key ever offered, all equal, whichever order the lanes of a step run in and however many rounds are allowed."""
    stats = []
    for order in ORDERS:
        s = HostSet(harness, 4096, order=order, max_rounds=max_rounds)
        C.run_case(cases[name], s.commit, s.lookup, (name, order, max_rounds))
        stats.append(s.stats())
        s.close()
    # the statistics do not depend on the order either, except the probe lengths (which slot a key's neighbour took)
    for st in stats[1:]:
        assert {k: st[k] for k in ("resident", "rounds", "tail")} == {k: stats[0][k] for k in ("resident", "rounds", "tail")}
    st = stats[0]
    if name == "chain":
        # a round decides the head of the chain and what hangs off it: 8 rounds leave most of 300 to the tail
        assert st["resident"] == 300 and st["rounds"] == max_rounds
        assert st["tail"] == 300 if max_rounds == 0 else st["tail"] > 200
    if name == "one_key":
        assert st["resident"] == 1
        assert (st["rounds"], st["tail"]) == {0: (0, 1000), 1: (1, 999), DEFAULT_ROUNDS: (2, 0)}[max_rounds]
    if name == "near_keys":
        assert st["resident"] == 20
    if name == "state_counts":
        assert st["resident"] == 1 + 63 + 64 + 65 + 257


def test_conflict_free_batch_takes_one_round(harness):
    batch = [([C.key_of("h", 2 * t), C.key_of("h", 2 * t + 1)], C.tx_id_of("h", t), t, True) for t in range(500)]
    s = HostSet(harness, 1000)
    C.run_case([batch], s.commit, s.lookup)
    st = s.stats()
    assert (st["resident"], st["rounds"], st["tail"]) == (1000, 1, 0)
    s.close()


WRAP_SEED = 5           # with this seed two of the 8 keys below hash to the last of the 16 slots: one of them wraps


def test_full_small_table_wraps_and_finds_every_key(harness):
    """Capacity 8 = 16 slots, filled to 8: a probe passes the table's last slot (the statistics say so) and every
    key is found with its record."""
    keys = [C.key_of("w", i) for i in range(8)]
    batch = [([k], C.tx_id_of("w", i), i, True) for i, k in enumerate(keys)]
    for order in ORDERS:
        s = HostSet(harness, 8, seed=WRAP_SEED, order=order)
        assert s.stats()["slots"] == 16
        C.run_case([batch], s.commit, s.lookup, order)
        st = s.stats()
        assert st["resident"] == 8 and st["wraps"] >= 1 and st["probe"] >= 2
        # full: one more state is refused before anything changes, outputs included
        rc, out = s.commit_rc(C.flatten([([C.key_of("w", 99)], C.tx_id_of("w", 99), 0, True)]), fill=0xEE)
        assert rc == -4 and out["tx_status"].tolist() == [0xEE] and out["cons_index"].tolist() == [0xEE]
        assert s.stats()["resident"] == 8
        s.close()


def test_growth_keeps_every_record(harness):
    """8 -> 1,024: every record survives byte for byte, the set goes on deciding as the oracle does."""
    keys = [C.key_of("w", i) for i in range(8)]
    first = [([k], C.tx_id_of("w", i), 100 + i, True) for i, k in enumerate(keys)]
    more = [([C.key_of("w", 8 + t), keys[t % 8]] if t % 5 == 0 else [C.key_of("w", 8 + t)], C.tx_id_of("w", 8 + t), t, True)
            for t in range(400)]
    for order in ORDERS:
        s = HostSet(harness, 8, seed=WRAP_SEED, order=order)
        oracle = C.InMemoryUniquenessProvider()
        C.assert_same(s.commit(C.flatten(first)), C.expect(oracle, first))
        before = s.lookup(C.keys_array(keys))
        assert s.reserve(4) == 0 and s.stats()["capacity"] == 8                  # never shrinks
        assert s.reserve(1024) == 0
        st = s.stats()
        assert (st["resident"], st["capacity"], st["slots"]) == (8, 1024, 2048)
        for a, b in zip(before, s.lookup(C.keys_array(keys))):
            assert np.array_equal(a, b)
        assert before[0].all()
        C.assert_same(s.commit(C.flatten(more)), C.expect(oracle, more))
        allk = keys + [C.key_of("w", 8 + t) for t in range(400)]
        for g, w in zip(s.lookup(C.keys_array(allk)), C.expect_lookup(oracle, allk)):
            assert np.array_equal(g, w)
        s.close()


def test_load_rejects_repeated_and_resident_keys(harness):
    keys = C.keys_array([C.key_of("l", i) for i in range(50)])
    ids = C.keys_array([C.tx_id_of("l", i) for i in range(50)])
    index, caller = np.arange(50, dtype=np.uint32) % 3, np.arange(50, dtype=np.uint32) + 9
    for order in ORDERS:
        s = HostSet(harness, 256, order=order)
        assert s.load(keys[:30], ids[:30], index[:30], caller[:30]) == 0
        assert s.stats()["resident"] == 30
        snapshot = s.lookup(keys)
        assert snapshot[0].tolist() == [1] * 30 + [0] * 20
        assert np.array_equal(snapshot[1][:30], ids[:30]) and np.array_equal(snapshot[2][:30], index[:30])
        assert np.array_equal(snapshot[3][:30], caller[:30])
        rep = np.concatenate([keys[30:40], keys[35:36]])                          # key 35 twice in one call
        assert s.load(rep, ids[:11], index[:11], caller[:11]) == -3
        res = np.concatenate([keys[40:50], keys[7:8]])                            # key 7 is resident
        assert s.load(res, ids[:11], index[:11], caller[:11]) == -3
        assert s.stats()["resident"] == 30
        for a, b in zip(snapshot, s.lookup(keys)):
            assert np.array_equal(a, b)                                           # unchanged
        assert s.load(keys[:1], ids[:1], index[:1], caller[:1]) == -3
        assert s.load(np.tile(keys[49:50], (300, 1)), np.tile(ids[:1], (300, 1)), np.zeros(300), np.zeros(300)) == -4
        # a loaded set decides like the oracle primed with the same rows
        oracle = C.InMemoryUniquenessProvider()
        oracle.commit_batch([([keys[i].tobytes()], C.SecureHash(ids[i].tobytes()), int(caller[i])) for i in range(30)])
        for i in range(30):                                                        # the rows' own input indices
            c = oracle.committed[keys[i].tobytes()]
            oracle.committed[keys[i].tobytes()] = type(c)(c.id, int(index[i]), c.requesting_party)
        batch = [([keys[i].tobytes(), keys[49 - i].tobytes()], C.tx_id_of("l2", i), i, True) for i in range(0, 50, 3)]
        C.assert_same(s.commit(C.flatten(batch)), C.expect(oracle, batch))
        s.close()


def test_argument_checks_without_a_device():
    """The C-ABI's checks that run before any device call: empty calls are CV_OK and touch nothing, counts past
    32 bits CV_E_TOO_LARGE, malformed ranges and missing arrays CV_E_ARGS, a null set or context CV_E_ARGS."""
    from corda_amd import native
    lib = native.load()
    OK, ARGS, TOO_LARGE = 0, -3, -5
    u32 = lambda *v: np.array(v, np.uint32)  # noqa: E731
    key, ids = np.zeros((4, 32), np.uint8), np.zeros((2, 32), np.uint8)
    st, sc = np.full(2, 9, np.uint8), np.full(4, 9, np.uint8)
    cid, cix, cc = np.full((4, 32), 9, np.uint8), np.full(4, 9, np.uint32), np.full(4, 9, np.uint32)

    def commit(ntx, k, b, i, c, sto=st, sco=sc, cido=cid):
        return lib.cv_uniq_commit_batch(None, ntx, _p(k), _p(b), _p(i), _p(c), None, _p(sto), _p(sco), _p(cido), _p(cix), _p(cc))

    h = ctypes.c_void_p(1)
    assert lib.cv_uniq_open(None, 0, 16, ctypes.byref(h)) == ARGS and not h.value
    assert lib.cv_uniq_open(None, 0, 16, None) == ARGS
    lib.cv_uniq_close(None)
    assert lib.cv_uniq_reserve(None, 16) == ARGS
    assert lib.cv_uniq_set_max_rounds(None, 1) == ARGS
    assert lib.cv_uniq_stats(None, _p(np.zeros(7, np.uint64)), 7) == ARGS
    assert commit(0, None, None, None, None, None, None, None) == OK
    assert commit(2, key, u32(0, 2, 4), ids, u32(1, 2)) == ARGS                   # well formed: the null set
    assert commit(2, key, u32(1, 2, 4), ids, u32(1, 2)) == ARGS                   # begin[0] != 0
    assert commit(2, key, u32(0, 3, 2), ids, u32(1, 2)) == ARGS                   # not monotone
    assert commit(2, None, u32(0, 2, 4), ids, u32(1, 2)) == ARGS                  # states without keys
    assert commit(2, key, None, ids, u32(1, 2)) == ARGS
    assert commit(2, key, u32(0, 2, 4), None, u32(1, 2)) == ARGS
    assert commit(2, key, u32(0, 2, 4), ids, None) == ARGS
    assert commit(2, key, u32(0, 2, 4), ids, u32(1, 2), sto=None) == ARGS
    assert commit(2, key, u32(0, 2, 4), ids, u32(1, 2), sco=None) == ARGS
    assert commit(2, key, u32(0, 2, 4), ids, u32(1, 2), cido=None) == ARGS
    assert commit(2, None, u32(0, 0, 0), ids, u32(1, 2), sco=None, cido=None) == ARGS   # no states: only the null set
    assert commit(1, key, u32(0, 0xffffffff), ids, u32(1)) == TOO_LARGE
    assert commit(0xffffffff, key, u32(0), ids, u32(1)) == TOO_LARGE
    found = np.full(4, 9, np.uint8)
    assert lib.cv_uniq_lookup(None, 0, None, None, None, None, None) == OK
    assert lib.cv_uniq_lookup(None, 4, _p(key), _p(found), _p(cid), _p(cix), _p(cc)) == ARGS
    assert lib.cv_uniq_lookup(None, 4, None, _p(found), _p(cid), _p(cix), _p(cc)) == ARGS
    assert lib.cv_uniq_lookup(None, 0xffffffff, _p(key), _p(found), _p(cid), _p(cix), _p(cc)) == TOO_LARGE
    assert lib.cv_uniq_load(None, 0, None, None, None, None) == OK
    assert lib.cv_uniq_load(None, 4, _p(key), _p(cid), _p(cix), _p(cc)) == ARGS
    assert lib.cv_uniq_load(None, 4, _p(key), None, _p(cix), _p(cc)) == ARGS
    assert lib.cv_uniq_load(None, 0xffffffff, _p(key), _p(cid), _p(cix), _p(cc)) == TOO_LARGE
    assert st.tolist() == [9, 9] and sc.tolist() == [9] * 4 and found.tolist() == [9] * 4 and (cid == 9).all()


def test_sanitizers_standalone_program():
    """tests/uniq_san.cpp (its own main: random batches with carry-over, the chain and growth against a sequential
    map) under ASan + UBSan, run as a subprocess: nothing is loaded into this process under a sanitizer."""
    exe = os.path.join(REPO, "tests", "_build", "uniq_san")
    src = os.path.join(REPO, "tests", "uniq_san.cpp")
    if _stale(exe, _deps(src, os.path.join(REPO, "tests", "uniq_harness.cpp"))):
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
