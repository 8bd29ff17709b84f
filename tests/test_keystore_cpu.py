"""The key store's core compiled for the CPU (corda_amd/csrc/cv_keystore.h through tests/keystore_harness.cpp) against
the Python oracle and sign_ref (tests/keystore_cases.py), exactly: every step's lanes run in ascending, descending and
one shuffled order, over tables forced small (capacity 8 = 16 slots, a probe that wraps past the last slot); in-call and
resident duplicates; the capacity refusal; growth; the status precedence of the builder's signing step; the C-ABI's
argument checks that need no device; and the same core under AddressSanitizer + UndefinedBehaviorSanitizer as a
stand-alone program (tests/keystore_san.cpp).  No GPU.

Reference: Services.kt:206-219, PersistentKeyManagementService.kt:40-66, CashFlow.kt:39-47, TransactionBuilder.kt:93-98.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ed25519_ref as E
import keystore_cases as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
ORDERS = (0, 1, 2)              # the harness's lane orders: ascending, descending, shuffled
NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1


def _deps(*srcs):
    csrc = os.path.join(REPO, "corda_amd", "csrc")
    return list(srcs) + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def harness():
    """tests/keystore_harness.cpp built as tests/test_uniq_cpu.py builds its harness."""
    lib = os.path.join(REPO, "tests", "_build", "libcvkeystore.so")
    src = os.path.join(REPO, "tests", "keystore_harness.cpp")
    if _stale(lib, _deps(src)):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-O2", "-std=c++17", "-fPIC",
                        "-shared", src, "-o", lib], check=True)
    h = ctypes.CDLL(lib)
    vp, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    h.hks_open.restype = vp
    h.hks_open.argtypes = [u64, u64]
    h.hks_close.argtypes = [vp]
    h.hks_stats.argtypes = [vp, vp]
    h.hks_reserve.argtypes = [vp, u64, ci]
    h.hks_add.argtypes = [vp, u32, vp, ci, vp, vp]
    h.hks_lookup.argtypes = [vp, u32, vp, ci, vp, vp, ci]
    h.hks_record.argtypes = [vp, u32, vp]
    h.hks_tx_gate.argtypes = [vp, u32, vp, vp, vp, ci] + [vp] * 5
    return h


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _rows(list_of_bytes):
    return np.frombuffer(b"".join(list_of_bytes), np.uint8).reshape(-1, 32).copy()


class HostStore:
    """One store of the harness with the calls of native.KeyStore."""

    def __init__(self, h, capacity, seed=0x243F6A8885A308D3, order=0):
        self.h, self.order = h, order
        self.p = h.hks_open(capacity, seed)

    def close(self):
        self.h.hks_close(self.p)

    def stats(self):
        out = np.zeros(4, np.uint64)
        self.h.hks_stats(self.p, _p(out))
        return dict(zip(("resident", "capacity", "slots", "probe"), map(int, out)))

    def add_rc(self, seeds, fill=0):
        seeds = _rows(seeds)
        n = len(seeds)
        pk, st = np.full((n, 32), fill, np.uint8), np.full(n, fill, np.uint8)
        rc = self.h.hks_add(self.p, n, _p(seeds), self.order, _p(pk), _p(st))
        return rc, pk, st

    def add(self, seeds):
        rc, pk, st = self.add_rc(seeds)
        assert rc == 0
        return pk, st

    def lookup(self, keys, present=1):
        keys = _rows(keys)
        n = len(keys)
        slot, flag = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        assert self.h.hks_lookup(self.p, n, _p(keys), self.order, _p(slot), _p(flag), present) == 0
        return slot, flag

    def record(self, slot):
        out = np.zeros(24, np.uint32)
        self.h.hks_record(self.p, int(slot), _p(out))
        b = out.tobytes()
        return b[:32], b[32:64], b[64:]

    def reserve(self, capacity):
        return self.h.hks_reserve(self.p, capacity, self.order)

    def tx_gate(self, txs):
        _, lb, pk, sb = K.flatten_txs(txs)
        ntx, ns = len(txs), max(len(pk), 1)
        slot, off, ln = np.full(ns, 7, np.uint32), np.full(ns, 7, np.uint64), np.full(ns, 7, np.uint32)
        st, fb = np.full(ntx, 7, np.uint8), np.full(ntx, 7, np.uint32)
        pkp = pk if len(pk) else np.zeros((1, 32), np.uint8)
        assert self.h.hks_tx_gate(self.p, ntx, _p(lb), _p(sb), _p(pkp), self.order, _p(slot), _p(off), _p(ln), _p(st), _p(fb)) == 0
        return slot[:len(pk)], off[:len(pk)], ln[:len(pk)], st, fb, sb


@pytest.fixture(scope="module")
def keys():
    """24 seeds with the oracle's expansion of each: (seed, a, prefix, public key)."""
    rng = np.random.default_rng(5016)
    out = []
    for _ in range(24):
        seed = rng.bytes(32)
        a, prefix, pk = E.seed_to_keypair(seed)
        out.append((seed, a.to_bytes(32, "little"), prefix, pk))
    return out


def _check_records(s, ks):
    """Every key of ks is resident and its slot holds the oracle's a | prefix | Abyte."""
    slot, found = s.lookup([k[3] for k in ks])
    assert found.tolist() == [1] * len(ks) and len(set(slot.tolist())) == len(ks)
    for sl, (_, a, prefix, pk) in zip(slot, ks):
        assert s.record(sl) == (a, prefix, pk)


def test_add_first_in_order_wins_in_every_lane_order(harness, keys):
    """One call of 14 seeds with repeats inside it, then a call that mixes resident keys, new keys and repeats: ADDED
    exactly at the first occurrence of a key that is not resident, pk_out for every record, whichever order the lanes
    of a step run in."""
    first = [0, 1, 2, 1, 3, 0, 4, 5, 5, 5, 6, 2, 7, 0]
    second = [8, 3, 9, 8, 10, 0, 11, 11]
    for order in ORDERS:
        s = HostStore(harness, 16, order=order)
        pk, st = s.add([keys[i][0] for i in first])
        assert [bytes(r) for r in pk] == [keys[i][3] for i in first]
        assert st.tolist() == [K.KS_PRESENT if i in first[:j] else K.KS_ADDED for j, i in enumerate(first)]
        assert s.stats()["resident"] == 8
        pk, st = s.add([keys[i][0] for i in second])
        assert [bytes(r) for r in pk] == [keys[i][3] for i in second]
        assert st.tolist() == [K.KS_ADDED, K.KS_PRESENT, K.KS_ADDED, K.KS_PRESENT, K.KS_ADDED, K.KS_PRESENT, K.KS_ADDED,
                               K.KS_PRESENT]
        assert s.stats()["resident"] == 12
        _check_records(s, keys[:12])
        assert s.lookup([keys[i][3] for i in (12, 0, 13)])[1].tolist() == [0, 1, 0]
        assert s.lookup([keys[i][3] for i in (12, 0, 13)], present=K.KS_OK)[1].tolist() == [K.KS_NO_KEY, K.KS_OK, K.KS_NO_KEY]
        s.close()


def _mix64(x):
    x ^= x >> 32
    x = x * 0xD6E8FEB86659FD93 & M64
    x ^= x >> 29
    x = x * 0x9E3779B97F4A7C15 & M64
    return x ^ (x >> 32)


def _home(pk: bytes, seed: int, mask: int) -> int:
    """cvu_hash's slot for a key (cv_uniq.h), restated."""
    w = np.frombuffer(pk, "<u8")
    h = seed
    for q in range(4):
        h = (_mix64(h ^ int(w[q])) + seed) & M64
    return h & mask


def test_full_small_table_wraps_and_finds_every_key(harness, keys):
    """Capacity 8 = 16 slots, filled to 8, with a table seed under which two keys hash to the LAST slot: one of them
    lies past the table's end, at the front.  Every key is found with its record; a ninth is refused before anything
    changes, outputs included."""
    pks = [k[3] for k in keys[:8]]
    homes = lambda sd: [_home(p, sd, 15) for p in pks]  # noqa: E731
    seed = next(sd for sd in range(1, 20000) if homes(sd).count(15) == 2 and 14 not in homes(sd))
    last = [i for i, p in enumerate(pks) if _home(p, seed, 15) == 15]
    for order in ORDERS:
        s = HostStore(harness, 8, seed=seed, order=order)
        assert s.stats()["slots"] == 16
        _, st = s.add([k[0] for k in keys[:8]])
        assert st.tolist() == [K.KS_ADDED] * 8
        slot, _ = s.lookup(pks)
        assert 15 in [int(slot[i]) for i in last] and any(int(slot[i]) < 8 for i in last)      # the probe wrapped
        assert s.stats()["resident"] == 8                           # a wrap is not counted: word 2 is the added count
        _check_records(s, keys[:8])
        assert s.stats()["probe"] >= 2
        rc, pk, st = s.add_rc([keys[8][0]], fill=0xEE)
        assert rc == -4 and (pk == 0xEE).all() and st.tolist() == [0xEE]
        rc, pk, st = s.add_rc([keys[0][0]], fill=0xEE)              # a repeat counts too: resident + n
        assert rc == -4 and st.tolist() == [0xEE]
        assert s.stats()["resident"] == 8
        _check_records(s, keys[:8])
        assert s.lookup([keys[8][3]])[1].tolist() == [0]
        s.close()


def test_growth_keeps_every_record(harness, keys):
    """8 -> 64: every record survives byte for byte, the store takes more keys and still refuses repeats."""
    for order in ORDERS:
        s = HostStore(harness, 8, seed=3, order=order)
        s.add([k[0] for k in keys[:8]])
        assert s.reserve(4) == 0 and s.stats()["capacity"] == 8                  # never shrinks
        assert s.reserve(64) == 0
        st = s.stats()
        assert (st["resident"], st["capacity"], st["slots"]) == (8, 64, 128)
        _check_records(s, keys[:8])
        _, st = s.add([k[0] for k in keys[4:24]])
        assert st.tolist() == [K.KS_PRESENT] * 4 + [K.KS_ADDED] * 16
        assert s.stats()["resident"] == 24
        _check_records(s, keys)
        s.close()


def _check_gate(s, txs, store, keys_by_pk, what):
    """The gate's outputs against sign_ref with a `sign` that names the signing key: statuses, first_bad, and per key
    the slot of ITS record, or none for every key of an abandoned transaction."""
    want = K.sign_ref(store, txs, lambda seed, msg: seed, id_of=lambda leaves: b"")
    slot, off, ln, st, fb, sb = s.tx_gate(txs)
    assert st.tolist() == [w[0] for w in want], what
    assert fb.tolist() == [w[1] for w in want], what
    for t, ((_, ks), w) in enumerate(zip(txs, want)):
        b = int(sb[t])
        assert off[b:b + len(ks)].tolist() == [32 * t] * len(ks) and ln[b:b + len(ks)].tolist() == [32] * len(ks)
        for j, k in enumerate(ks):
            if w[0] != K.ST_OK:
                assert slot[b + j] == NONE, (what, t, j)
            else:
                assert s.record(slot[b + j]) == keys_by_pk[k], (what, t, j)


def test_status_precedence_cases(harness, keys):
    """Every named case of keystore_cases.precedence_txs: the expected (status, first_bad) as literals, sign_ref's as
    well, in every lane order; among them the empty transaction whose key 0 is absent (NO_KEY) and the one whose key 0
    is present (EMPTY), and the three-key transaction whose key 2 repeats key 0 while key 1 is absent: NO_KEY at 1."""
    present, absent = [k[3] for k in keys[:6]], [k[3] for k in keys[6:9]]
    store = {k[3]: k[0] for k in keys[:6]}
    by_pk = {k[3]: (k[1], k[2], k[3]) for k in keys}
    cases = K.precedence_txs(present, absent)
    assert set(cases) == set(K.PRECEDENCE_EXPECT)
    names = list(cases)
    txs = [cases[n] for n in names]
    got = K.sign_ref(store, txs, lambda seed, msg: seed)
    assert [(g[0], g[1]) for g in got] == [K.PRECEDENCE_EXPECT[n] for n in names]
    assert K.PRECEDENCE_EXPECT["no_key_before_dup"] == (K.ST_NO_KEY, 1)
    for order in ORDERS:
        s = HostStore(harness, 8, seed=11, order=order)
        s.add([k[0] for k in keys[:6]])
        _check_gate(s, txs, store, by_pk, order)
        s.close()


def test_random_transactions_against_sign_ref(harness, keys):
    rng = np.random.default_rng(93)
    present, absent = [k[3] for k in keys[:16]], [k[3] for k in keys[16:]]
    store = {k[3]: k[0] for k in keys[:16]}
    by_pk = {k[3]: (k[1], k[2], k[3]) for k in keys}
    txs = K.random_txs(rng, 300, present, absent)
    want = K.sign_ref(store, txs, lambda seed, msg: seed)
    assert {w[0] for w in want} == {K.ST_OK, K.ST_NO_KEY, K.ST_ALREADY_SIGNED, K.ST_EMPTY}
    for order in ORDERS:
        s = HostStore(harness, 16, seed=order + 1, order=order)      # 32 slots, half full
        s.add([k[0] for k in keys[:16]])
        _check_gate(s, txs, store, by_pk, order)
        s.close()


def test_argument_checks_without_a_device():
    """The C-ABI's checks that run before any device call: empty calls are CV_OK and touch nothing, counts past
    32 bits CV_E_TOO_LARGE, malformed ranges, records past the arena and missing arrays CV_E_ARGS, a null store or
    context CV_E_ARGS."""
    from corda_amd import native
    lib = native.load()
    OK, ARGS, TOO_LARGE = 0, -3, -5
    u32 = lambda *v: np.array(v, np.uint32)  # noqa: E731
    u64 = lambda *v: np.array(v, np.uint64)  # noqa: E731
    P = native._p
    h = ctypes.c_void_p(1)
    assert lib.cv_keystore_open(None, 0, 16, ctypes.byref(h)) == ARGS and not h.value
    assert lib.cv_keystore_open(None, 0, 16, None) == ARGS
    assert lib.cv_keystore_close(None) is None
    assert lib.cv_keystore_reserve(None, 16) == ARGS
    assert lib.cv_keystore_stats(None, P(np.zeros(4, np.uint64)), 4) == ARGS
    seed, pk, st = np.zeros((2, 32), np.uint8), np.full((2, 32), 9, np.uint8), np.full(2, 9, np.uint8)
    sig = np.full((2, 64), 9, np.uint8)
    assert lib.cv_keystore_add(None, 0, None, None, None) == OK
    assert lib.cv_keystore_add(None, 2, P(seed), P(pk), P(st)) == ARGS                 # well formed: the null store
    assert lib.cv_keystore_add(None, 2, None, P(pk), P(st)) == ARGS
    assert lib.cv_keystore_add(None, 0xffffffff, P(seed), P(pk), P(st)) == TOO_LARGE
    assert lib.cv_keystore_contains(None, 0, None, None) == OK
    assert lib.cv_keystore_contains(None, 2, P(seed), P(st)) == ARGS
    assert lib.cv_keystore_contains(None, 2, P(seed), None) == ARGS
    assert lib.cv_keystore_contains(None, 0xffffffff, P(seed), P(st)) == TOO_LARGE
    arena = np.zeros(64, np.uint8)
    sign = lambda n, off, ln, bound=64, a=arena: lib.cv_keystore_sign(  # noqa: E731
        None, n, P(seed), P(a), bound, P(off), P(ln), P(sig), P(st))
    assert sign(0, None, None) == OK
    assert sign(2, u64(0, 32), u32(32, 32)) == ARGS                                     # well formed: the null store
    assert sign(2, u64(0, 32), u32(32, 33)) == ARGS                                     # past the arena
    assert sign(2, u64(0, 2 ** 64 - 8), u32(32, 32)) == ARGS                            # wraps
    assert sign(2, u64(0, 32), u32(32, 32), a=None) == ARGS
    assert sign(2, None, u32(32, 32)) == ARGS
    assert sign(0xffffffff, u64(0, 32), u32(32, 32)) == TOO_LARGE
    ids, fb = np.full((2, 32), 9, np.uint8), np.full(2, 9, np.uint32)
    off, ln = u64(0, 10, 20), u32(10, 10, 10)

    def txs(ntx, lb, nsig, sb, bound=64, o=off, ll=ln, stat=st, idsp=ids, sigp=sig, pkp=seed):
        return lib.cv_sign_transactions(None, None, ntx, P(arena), bound, P(o), P(ll), P(lb), nsig, P(pkp), P(sb), P(stat),
                                        P(idsp), P(sigp), P(fb))

    assert txs(0, None, 0, None) == OK
    assert txs(2, u32(0, 2, 3), 2, u32(0, 1, 2)) == ARGS                                # well formed: null ctx and store
    assert txs(2, u32(1, 2, 3), 2, u32(0, 1, 2)) == ARGS                                # begin[0] != 0
    assert txs(2, u32(0, 3, 2), 2, u32(0, 1, 2)) == ARGS                                # not monotone
    assert txs(2, u32(0, 2, 3), 2, u32(0, 2, 1)) == ARGS
    assert txs(2, u32(0, 2, 3), 2, u32(0, 1, 1)) == ARGS                                # ends short of nsig
    assert txs(2, u32(0, 2, 3), 2, u32(0, 1, 2), bound=29) == ARGS                      # a leaf past the arena
    assert txs(2, u32(0, 2, 3), 2, u32(0, 1, 2), o=u64(0, 10, 2 ** 64 - 4)) == ARGS     # wraps
    assert txs(2, u32(0, 2, 3), 2, u32(0, 1, 2), stat=None) == ARGS
    assert txs(2, u32(0, 2, 3), 2, u32(0, 1, 2), idsp=None) == ARGS
    assert txs(2, u32(0, 2, 3), 2, u32(0, 1, 2), sigp=None) == ARGS
    assert txs(2, u32(0, 2, 3), 2, u32(0, 1, 2), pkp=None) == ARGS
    assert txs(2, None, 2, u32(0, 1, 2)) == ARGS
    assert txs(0xffffffff, u32(0), 0, u32(0)) == TOO_LARGE
    assert txs(1, u32(0, 0xffffffff), 0, u32(0, 0)) == TOO_LARGE
    assert (pk == 9).all() and (st == 9).all() and (sig == 9).all() and (ids == 9).all() and (fb == 9).all()
    for name in ("cv_keystore_open", "cv_keystore_close", "cv_keystore_reserve", "cv_keystore_add", "cv_keystore_contains",
                 "cv_keystore_sign", "cv_keystore_stats", "cv_sign_transactions"):
        assert name in native.EXPORTED


def test_sanitizers_standalone_program():
    """tests/keystore_san.cpp (its own main: random adds with repeats on a store that has to grow, lookups and the
    transactions' gate against a sequential map) under ASan + UBSan, run as a subprocess: nothing is loaded into this
    process under a sanitizer."""
    exe = os.path.join(REPO, "tests", "_build", "keystore_san")
    src = os.path.join(REPO, "tests", "keystore_san.cpp")
    if _stale(exe, _deps(src, os.path.join(REPO, "tests", "keystore_harness.cpp"))):
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
