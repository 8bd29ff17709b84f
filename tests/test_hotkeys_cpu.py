"""The hot-key route's steps compiled for the CPU (corda_amd/csrc/cv_hotkeys.h through tests/hotkeys_harness.cpp) against
the classification in plain Python (tests/hotkeys_cases.py): every case with the lanes of every step run in ascending,
descending and one shuffled order, with and without the tally's wave election; the merge with the two verifies
replaced by a function of a gathered row's bytes; the workspace's size and alignment; the argument checks of
cv_ed25519_verify_device_hotkeys that need no device; and the same code under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/hotkeys_san.cpp).  No GPU.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hotkeys_cases as C
import keydedupe_cases as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
ORDERS = (0, 1, 2)              # the harness's lane orders: ascending, descending, shuffled
CSRC = os.path.join(REPO, "corda_amd", "csrc")
LAYOUT = ("dedupe", "keys", "key_index", "nkeys", "count", "cand", "cls", "stat", "head", "hot_keys", "rank", "perm", "g_pk",
          "g_sig", "g_off", "g_len", "g_kidx", "bm_hot", "bm_cold", "sub_status", "bytes")


def _deps(*srcs):
    heads = ("cv_hotkeys.h", "cv_keydedupe.h", "cv_uniq.h", "cv_table.h")
    return list(srcs) + [os.path.join(CSRC, h) for h in heads] + [os.path.join(REPO, "tests", "keydedupe_harness.cpp")]


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def harness():
    """tests/hotkeys_harness.cpp built as tests/test_keydedupe_cpu.py builds its harness."""
    lib = os.path.join(REPO, "tests", "_build", "libcvhotkeys.so")
    src = os.path.join(REPO, "tests", "hotkeys_harness.cpp")
    if _stale(lib, _deps(src)):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-O2", "-std=c++17", "-fPIC",
                        "-shared", src, "-o", lib], check=True)
    h = ctypes.CDLL(lib)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    h.hhk_run.argtypes = [u32, vp, vp, vp, vp, u32, u32, ctypes.c_int, ctypes.c_int, u64] + [vp] * 7
    h.hhk_run.restype = ctypes.c_int
    h.hhk_workspace.argtypes = [u64]
    h.hhk_workspace.restype = u64
    h.hhk_rows.argtypes = [u64, u32, u32]
    h.hhk_rows.restype = u64
    h.hhk_layout.argtypes = [u64, vp]
    h.hhk_layout.restype = None
    return h


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def records(pk, seed=1):
    """Signature rows, offsets and lengths for pk's records: arbitrary bytes, the stand-in verify only hashes them."""
    rng = np.random.default_rng(seed)
    n = len(pk)
    return (rng.integers(0, 1 << 32, (n, 16), dtype=np.uint64).astype(np.uint32),
            rng.integers(0, 1 << 40, n, dtype=np.uint64), rng.integers(0, 5000, n, dtype=np.uint64).astype(np.uint32))


def fake(pk, sig, off, ln):
    """hhk_fake of tests/hotkeys_harness.cpp -> (verdict bits, status bytes)."""
    kw = np.ascontiguousarray(pk, np.uint8).reshape(-1, 32).view(np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = np.uint64(5) * off + np.uint64(7) * ln.astype(np.uint64)
        h = h + (kw * np.arange(1, 9, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
        h = h + (sig.astype(np.uint64) * (3 * np.arange(16, dtype=np.uint64) + 2)).sum(axis=1, dtype=np.uint64)
    h ^= h >> np.uint64(17)
    return (h & np.uint64(1)).astype(bool), ((h >> np.uint64(1)) & np.uint64(1)).astype(np.uint8)


def run(h, pk, hot_min, hot_cap, order, elect=0, with_status=True, seed=0x9e3779b97f4a7c15):
    n = len(pk)
    w = K.words(pk)
    sig, off, ln = records(pk)
    cls, hotnum, perm = (np.full(n, 0xEEEEEEEE, np.uint32) for _ in range(3))
    head, hot_keys = np.zeros(4, np.uint32), np.full((n, 32), 0xEE, np.uint8)
    words = (n + 63) // 64
    bitmap = np.full(words + 1, 0xEEEEEEEEEEEEEEEE, np.uint64)                 # one guard word behind
    status = np.full(n + 8, 0xEE, np.uint8) if with_status else None
    rc = h.hhk_run(n, _p(w), _p(sig), _p(off), _p(ln), hot_min, hot_cap, order, elect, seed, _p(cls), _p(hotnum), _p(perm),
                   _p(head), _p(hot_keys), _p(bitmap), _p(status))
    assert rc == 0, rc
    return dict(cls=cls, hotnum=hotnum, perm=perm, head=head, hot_keys=hot_keys, bitmap=bitmap, status=status,
                fake=fake(pk, sig, off, ln))


def check(got, pk, hot_min, hot_cap, what):
    n = len(pk)
    cls, hotnum, perm, nhot = C.reference(pk, hot_min, hot_cap)
    keys, _, nk = K.reference(pk)
    hk = int((cls != C.COLD).sum())
    assert got["head"].tolist() == [nk, hk, 1, nhot], (what, got["head"])
    assert (nk, hk, nhot, n - nhot) == C.route(pk, hot_min, hot_cap)
    assert np.array_equal(got["cls"][:nk], cls) and (got["cls"][nk:] == C.COLD).all(), what
    assert np.array_equal(got["hotnum"][:nk], hotnum), what
    assert np.array_equal(got["perm"], perm), what
    assert np.array_equal(got["hot_keys"][:hk], keys[cls != C.COLD]), what        # first-seen order among the hot keys
    assert (got["hot_keys"][hk:] == 0xEE).all(), what                             # rows from the count on are not written
    bits, st = got["fake"]
    want = np.zeros(((n + 63) // 64) * 64, bool)
    want[:n] = bits
    words = np.packbits(want.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).ravel()
    assert np.array_equal(got["bitmap"][:-1], words), what                        # whole words, zero tail bits
    assert got["bitmap"][-1] == 0xEEEEEEEEEEEEEEEE, what                          # and not a word more
    if got["status"] is not None:
        assert np.array_equal(got["status"][:n], st) and (got["status"][n:] == 0xEE).all(), what


@pytest.fixture(scope="module")
def cases():
    return C.cases()


@pytest.mark.parametrize("name", list(C.cases()))
def test_cases_in_every_lane_order(harness, cases, name):
    """The classes, hotnum, perm, the counts, the hot key rows and the merged outputs equal the reference, whichever
    order the lanes run in, with the tally lane by lane and wave by wave."""
    pk, hot_min, cap = cases[name]
    for order in ORDERS:
        for elect in (0, 1):
            check(run(harness, pk, hot_min, cap, order, elect), pk, hot_min, cap, (name, order, elect))


def test_the_cases_cover_what_they_name(cases):
    for hm in (2, 3, 8):
        pk, hot_min, cap = cases[f"around_min{hm}"]
        _, index, nk = K.reference(pk)
        count = np.bincount(index)
        assert sorted(count.tolist()) == sorted([hm - 1, hm, hm + 1, 1, 1, 1])
        cls = C.reference(pk, hot_min, cap)[0]
        assert ((cls != C.COLD) == (count >= hm)).all() and (cls != C.COLD).sum() == 2
    pk, hot_min, cap = cases["first_hot_record_at_index_0"]
    assert C.reference(pk, hot_min, cap)[2][0] == 0 and 0 < C.reference(pk, hot_min, cap)[3] < len(pk)
    pk, hot_min, cap = cases["hot_records_at_the_end"]
    cls, _, perm, nhot = C.reference(pk, hot_min, cap)
    assert nhot == 3 and perm[-1] == 2 and perm[0] == 3 and (perm[:-3] >= 3).all()
    pk, hot_min, cap = cases["first_hot_record_at_the_last_index"]
    cls, _, perm, nhot = C.reference(pk, hot_min, cap)
    assert nhot == len(pk) and perm[-1] == len(pk) - 1 and cls.tolist() == [0, 1]
    pk, hot_min, cap = cases["more_candidates_than_cap"]
    cls, hotnum, _, nhot = C.reference(pk, hot_min, cap)
    cand = np.bincount(K.reference(pk)[1]) >= 2
    assert cand.sum() == 9 and (cls != C.COLD).sum() == 4 and (cls[cand][:4] != C.COLD).all() and (cls[cand][4:] == C.COLD).all()
    pk, hot_min, cap = cases["all_distinct/min1"]
    assert C.route(pk, hot_min, cap) == (300, 300, 300, 0)
    pk, hot_min, cap = cases["all_distinct/min301"]
    assert C.route(pk, hot_min, cap) == (300, 0, 0, 300)
    assert C.route(*cases["default_min"]) == (5, 2, 17, 9)


@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129])
def test_merge_at_the_word_boundaries(harness, n):
    """The merge with the two verifies replaced by a function of the gathered row's bytes: bitmap words, zero tail
    bits, the status copy, with and without a status array, around one and two words."""
    pk = K.pool(("merge", n), 12)[np.random.default_rng(n).integers(0, 12, n)]
    pk[-1] = K.key("merge", n, "once")                       # a cold record in the last lane
    for hot_min in (2, 6):
        nk, hk, nhot, ncold = C.route(pk, hot_min)
        assert 0 < nhot < n
        for order in ORDERS:
            for with_status in (True, False):
                check(run(harness, pk, hot_min, C.CAP, order, with_status=with_status), pk, hot_min, C.CAP, (n, hot_min, order))


def test_the_result_does_not_depend_on_the_seed(harness, cases):
    pk, hot_min, cap = cases["past_two_blocks"]
    for seed in (1, 0xdeadbeefcafef00d):
        check(run(harness, pk, hot_min, cap, 2, seed=seed), pk, hot_min, cap, seed)


def test_workspace_size_and_alignment(harness):
    """cv_ed25519_verify_hotkeys_workspace is the header's layout; every piece is 16-byte aligned, head lies directly
    before hot_keys (one copy reads both back), and the cold sub-batch's bases — 32, 64 and 8 bytes per hot record past
    the gathered arrays — keep the 16- and 8-byte alignment the verify kernels need for every count of hot records."""
    from corda_amd import native
    for n in (1, 2, 63, 64, 65, 1024, 1025, 5000, 1 << 20, (1 << 20) + 1, (1 << 30) + 7, 0xfffffffe):
        out = np.zeros(21, np.uint64)
        harness.hhk_layout(n, _p(out))
        L = dict(zip(LAYOUT, (int(v) for v in out)))
        assert native.verify_hotkeys_workspace(n) == L["bytes"] == harness.hhk_workspace(n)
        assert all(v % 16 == 0 for v in L.values())
        offs = [L[k] for k in LAYOUT]
        assert offs == sorted(offs) and L["dedupe"] == 0 and L["keys"] >= native.dedupe_keys_workspace(n)
        assert L["hot_keys"] == L["head"] + 16
        sizes = dict(keys=32, key_index=4, count=4, cand=4, cls=4, hot_keys=32, rank=4, perm=4, g_pk=32, g_sig=64, g_off=8,
                     g_len=4, g_kidx=4, sub_status=1)
        for k, per in sizes.items():
            assert offs[LAYOUT.index(k) + 1] - L[k] >= per * n, (n, k)
        assert L["bm_cold"] - L["bm_hot"] >= 8 * ((n + 63) // 64) and L["sub_status"] - L["bm_cold"] >= 8 * ((n + 63) // 64)
        for nhot in (1, 3, 63, 64, 65, n - 1):
            assert (L["g_pk"] + 32 * nhot) % 16 == 0 and (L["g_sig"] + 64 * nhot) % 16 == 0
            assert (L["g_off"] + 8 * nhot) % 8 == 0 and (L["g_len"] + 4 * nhot) % 4 == 0
    assert native.verify_hotkeys_workspace(0xffffffff) == 0
    # the rows read back: no more keys than n / hot_min can be candidates, no more than the capacity hot
    assert harness.hhk_rows(699, 8, 16384) == 87 and harness.hhk_rows(1 << 20, 1, 16384) == 16384
    assert harness.hhk_rows(100, 101, 16384) == 0 and harness.hhk_rows(100, 2, 4) == 4


def test_argument_checks_without_a_device():
    """cv_ed25519_verify_device_hotkeys's checks run before any device work: n == 0 is CV_OK and touches nothing,
    n past 0xfffffffe is CV_E_TOO_LARGE, a null context is CV_E_ARGS."""
    from corda_amd import native
    lib = native.load()
    buf = np.zeros(64, np.uint8)
    p = native._p(buf)
    route = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    f = lib.cv_ed25519_verify_device_hotkeys
    assert f(None, 0, 1, p, p, p, p, p, p, p, 0, p, None, route) == -3
    assert f(None, 0, 0, None, None, None, None, None, None, None, 0, None, None, route) == 0
    assert f(None, 0, 0xffffffff, p, p, p, p, p, p, p, 0, p, None, route) == -5
    assert f(None, 0, 0xfffffffe, p, p, p, p, p, p, p, 0, p, None, route) == -3
    assert list(route) == [7, 7, 7, 7] and not buf.any()
    assert native.verify_hotkeys_workspace(0xffffffff) == 0 and native.verify_hotkeys_workspace(1) > 0
    assert "cv_ed25519_verify_device_hotkeys" in native.EXPORTED


def test_sanitizers_standalone_program():
    """tests/hotkeys_san.cpp (its own main: batches against a std::map restatement, every order, with and without the
    election, with and without a status array) under ASan + UBSan, run as a subprocess: nothing is loaded into this
    process under a sanitizer."""
    exe = os.path.join(REPO, "tests", "_build", "hotkeys_san")
    src = os.path.join(REPO, "tests", "hotkeys_san.cpp")
    if _stale(exe, _deps(src, os.path.join(REPO, "tests", "hotkeys_harness.cpp"))):
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
