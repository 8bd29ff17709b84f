"""The device key dedupe compiled for the CPU (corda_amd/csrc/cv_keydedupe.h through tests/keydedupe_harness.cpp)
against first-seen numbering in plain Python (tests/keydedupe_cases.py): every case with the lanes of every step run in
ascending, descending and one shuffled order; tables forced down to the next power of two >= n, full or nearly so,
under a seed whose probes pass the last slot; the argument checks of cv_ed25519_dedupe_keys_device that need no device;
and the same code under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program
(tests/keydedupe_san.cpp).  No GPU.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import keydedupe_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
ORDERS = (0, 1, 2)              # the harness's lane orders: ascending, descending, shuffled
SEEDS = (1, 0x9e3779b97f4a7c15, 0xdeadbeefcafef00d)
CSRC = os.path.join(REPO, "corda_amd", "csrc")
POISON = 0xEE


def _deps(*srcs):
    return list(srcs) + [os.path.join(CSRC, h) for h in ("cv_keydedupe.h", "cv_uniq.h", "cv_table.h")]


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def harness():
    """tests/keydedupe_harness.cpp built as tests/test_resolve_cpu.py builds its harness."""
    lib = os.path.join(REPO, "tests", "_build", "libcvkeydedupe.so")
    src = os.path.join(REPO, "tests", "keydedupe_harness.cpp")
    if _stale(lib, _deps(src)):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-O2", "-std=c++17", "-fPIC",
                        "-shared", src, "-o", lib], check=True)
    h = ctypes.CDLL(lib)
    vp = ctypes.c_void_p
    h.hkd_run.argtypes = [ctypes.c_uint32, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, vp, vp, vp, vp]
    h.hkd_run.restype = ctypes.c_int
    h.hkd_slots.argtypes = [ctypes.c_uint64]
    h.hkd_slots.restype = ctypes.c_uint64
    h.hkd_workspace.argtypes = [ctypes.c_uint64]
    h.hkd_workspace.restype = ctypes.c_uint64
    return h


@pytest.fixture(scope="module")
def cases():
    """Every case with its reference, computed once."""
    return {name: (pk, C.reference(pk)) for name, pk in C.cases().items()}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run(h, pk, order, seed=SEEDS[1], slots=0):
    """The steps in `order` -> (keys, key_index, nkeys, keys rows past nkeys, wrapped), the outputs poisoned before."""
    n = len(pk)
    w = C.words(pk)
    keys, index = np.full((n, 32), POISON, np.uint8), np.full(n, 0xEEEEEEEE, np.uint32)
    nkeys, wrapped = np.full(1, 0xEEEEEEEE, np.uint32), np.zeros(1, np.int32)
    rc = h.hkd_run(n, _p(w), seed, slots, order, _p(keys), _p(index), _p(nkeys), _p(wrapped))
    assert rc == 0, rc
    nk = int(nkeys[0])
    return keys[:nk], index, nk, keys[nk:], int(wrapped[0])


def same(got, want, what):
    keys, index, nk, rest, _ = got
    assert nk == want[2], (what, nk, want[2])
    assert np.array_equal(keys, want[0]), what
    assert np.array_equal(index, want[1]), what
    assert (rest == POISON).all(), what                # rows from nkeys on are not written


def small(n):
    return 1 << max(0, (n - 1).bit_length())


@pytest.mark.parametrize("name", list(C.cases()))
def test_cases_in_every_lane_order(harness, cases, name):
    """keys, key_index and nkeys equal the reference array for array, whichever order the lanes run in."""
    pk, want = cases[name]
    for order in ORDERS:
        same(run(harness, pk, order), want, (name, order))


@pytest.mark.parametrize("name", list(C.cases()))
def test_small_tables_collide_fill_and_wrap(harness, cases, name):
    """Slots = the next power of two >= n: the all-distinct cases fill it to the last slot or nearly.  The result
    changes neither with the seed nor with the order, and where the distinct keys fill more than half of the table
    some seed's probes pass the last slot."""
    pk, want = cases[name]
    n = len(pk)
    slots = small(n)
    assert n <= slots < 2 * max(n, 1) and slots < harness.hkd_slots(n)
    wrapped = 0
    for seed in SEEDS + tuple(range(2, 34)):
        for order in ORDERS if seed in SEEDS else (2,):
            got = run(harness, pk, order, seed=seed, slots=slots)
            same(got, want, (name, seed, order))
            wrapped += got[4]
    if want[2] >= 2 and 2 * want[2] > slots:
        assert wrapped > 0, name


def test_a_full_table(harness):
    """256 distinct keys in 256 slots: every probe loop ends within the slot count without an empty slot to stop at."""
    pk = C.pool("full", 256)
    want = C.reference(pk)
    for order in ORDERS:
        got = run(harness, pk, order, slots=256)
        same(got, want, order)
        assert got[4] == 1                             # a full table: some key lies below its home slot


def test_the_cases_cover_what_they_name(cases):
    pk, (keys, index, nk) = cases["differ_in_byte_31"]
    assert nk == 5 and (keys[:, :31] == keys[0, :31]).all() and len(set(keys[:, 31].tolist())) == 5
    pk, (keys, index, nk) = cases["differ_in_byte_0"]
    assert nk == 5 and (keys[:, 1:] == keys[0, 1:]).all() and len(set(keys[:, 0].tolist())) == 5
    pk, (keys, index, nk) = cases["first_occurrence_at_the_last_index"]
    assert index[-1] == nk - 1 and (index[:-1] < nk - 1).all()
    pk, (keys, index, nk) = cases["only_repeat_at_the_last_index"]
    assert np.flatnonzero(index == index[-1]).tolist() == [17, len(pk) - 1]
    assert cases["signed_pool_of_4"][1][2] == 4 and len(cases["signed_pool_of_4"][0]) == 5000
    assert cases["all_equal"][1][2] == 1 and cases["all_distinct"][1][2] == 300 and cases["alternating"][1][2] == 2
    pk, (keys, index, nk) = cases["bad_keys_repeated"]
    assert nk >= 4 and len(pk) >= 3 * nk - 6


def test_two_blocks_of_the_compaction(harness):
    """More rows than one block of the compaction (CVD_SPAN = 1024) and than two: the harness scans block by block."""
    for n in (1023, 1024, 1025, 2500):
        pk = C.pool("blocks", 700)[np.random.default_rng(n).integers(0, 700, n)]
        want = C.reference(pk)
        for order in ORDERS:
            same(run(harness, pk, order), want, (n, order))


def test_workspace_size(harness):
    """cv_ed25519_dedupe_keys_workspace is the header's layout: the table of at least 2 n slots and the arrays behind."""
    from corda_amd import native
    for n in (1, 2, 63, 1024, 1025, 5000, 1 << 20, (1 << 20) + 1, (1 << 30) + 7, 0xfffffffe):
        want = harness.hkd_workspace(n)
        assert native.dedupe_keys_workspace(n) == want
        slots = harness.hkd_slots(n)
        assert slots >= 2 * n and slots & (slots - 1) == 0 and slots < 4 * n + 2 and want >= 4 * slots + 8 * n
    assert native.dedupe_keys_workspace(0xffffffff) == 0


def test_argument_checks_without_a_device():
    """cv_ed25519_dedupe_keys_device's checks run before any device work: a null context is CV_E_ARGS, n == 0 is CV_OK
    and touches nothing, n past 0xfffffffe is CV_E_TOO_LARGE; the new option has a name and option 24 does not exist."""
    from corda_amd import native
    lib = native.load()
    buf = np.zeros(64, np.uint8)
    p = native._p(buf)
    assert lib.cv_ed25519_dedupe_keys_device(None, 0, 1, p, p, p, p, p, None) == -3
    assert lib.cv_ed25519_dedupe_keys_device(None, 0, 0, None, None, None, None, None, None) == 0
    assert lib.cv_ed25519_dedupe_keys_device(None, 0, 0xffffffff, p, p, p, p, p, None) == -5
    assert lib.cv_ed25519_dedupe_keys_device(None, 0, 0xfffffffe, p, p, p, p, p, None) == -3
    assert native.OPTIONS["fused_keyed"] == 23 and max(native.OPTIONS.values()) == 23
    assert lib.cv_set_option(None, 23, 1) == -3


def test_sanitizers_standalone_program():
    """tests/keydedupe_san.cpp (its own main: the cases against a std::map, every order, seed and table size) under
    ASan + UBSan, run as a subprocess: nothing is loaded into this process under a sanitizer."""
    exe = os.path.join(REPO, "tests", "_build", "keydedupe_san")
    src = os.path.join(REPO, "tests", "keydedupe_san.cpp")
    if _stale(exe, _deps(src, os.path.join(REPO, "tests", "keydedupe_harness.cpp"))):
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
