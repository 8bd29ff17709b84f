"""The decisions of cv_notarise_batch compiled for the CPU (corda_amd/csrc/cv_notary.h through
tests/notary_harness.cpp) against the restatement of NotaryFlow.Service.call + ValidatingNotaryFlow.beforeCommit in
tests/notarise_cases.py: the gate, the state-key gather and finalise with the lanes of every step run in ascending,
descending and one shuffled order; the C-ABI's argument checks that need no device; and the same code under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program (tests/notary_san.cpp).  No GPU.

Reference: NotaryFlow.kt:96-146, ValidatingNotaryFlow.kt:24-45, SignedTransaction.kt:34-38,58-93.
"""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import notarise_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
ORDERS = (0, 1, 2)              # the harness's lane orders: ascending, descending, shuffled


def _deps(*srcs):
    return list(srcs) + [os.path.join(REPO, "corda_amd", "csrc", "cv_notary.h")]


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def harness():
    """tests/notary_harness.cpp built as tests/test_uniq_cpu.py builds its harness."""
    lib = os.path.join(REPO, "tests", "_build", "libcvnotary.so")
    src = os.path.join(REPO, "tests", "notary_harness.cpp")
    if _stale(lib, _deps(src)):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-O2", "-std=c++17", "-fPIC",
                        "-shared", src, "-o", lib], check=True)
    h = ctypes.CDLL(lib)
    vp = ctypes.c_void_p
    h.hnt_gate.argtypes = [ctypes.c_uint32, ctypes.c_int] + [vp] * 9 + [ctypes.c_int] + [vp] * 3
    h.hnt_gate.restype = None
    h.hnt_gather.argtypes = [ctypes.c_uint32, vp, vp, ctypes.c_int, vp]
    h.hnt_gather.restype = None
    h.hnt_final.argtypes = [ctypes.c_uint32, vp, vp, ctypes.c_int] + [vp] * 4
    h.hnt_final.restype = ctypes.c_uint32
    return h


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run_gate(h, f, validating, order, with_pre=True):
    n = f["ntx"]
    pre, en, fb = np.full(n, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8), np.full(n, 0xEEEEEEEE, np.uint32)
    h.hnt_gate(n, validating, _p(f["mstatus"]), _p(f["id"]), _p(f["claimed"]), _p(f["tx_pre"]) if with_pre else None,
               _p(f["tx_sig_begin"]), _p(f["bitmap"]), _p(f["sig_status"]), _p(f["sig_pre"]) if with_pre else None,
               _p(f["ck"]), order, _p(pre), _p(en), _p(fb))
    return pre, en, fb


def run_final(h, pre, ust, order):
    n = len(pre)
    out, lst = np.full(n, 0xEE, np.uint8), np.full(n, 0xEEEEEEEE, np.uint32)
    off, ln = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    cnt = h.hnt_final(n, _p(pre), _p(ust), order, _p(out), _p(lst), _p(off), _p(ln))
    return out, lst[:cnt], off[:cnt], ln[:cnt]


@pytest.mark.parametrize("validating", [1, 0])
@pytest.mark.parametrize("name", list(C.CASES))
def test_cases_in_every_lane_order(harness, name, validating):
    """Outcome, first_bad, enable and the accepted list equal the restatement's, whichever order the lanes run in.  The
    uniqueness status between gate and finalise is the sequential provider's over the transactions the gate enabled."""
    txs, resident = C.CASES[name]()
    f = C.flatten(txs, validating)
    want_pre, want_en, want_fb = C.gate(txs, validating)
    want = C.notarise(txs, validating, resident)
    ust = np.where(want_en == 0, C.UNIQ_SKIPPED, np.where(want["outcome"] == C.CONFLICT, C.UNIQ_CONFLICT, C.UNIQ_OK)).astype(np.uint8)
    for order in ORDERS:
        pre, en, fb = run_gate(harness, f, validating, order)
        assert np.array_equal(pre, want_pre), (name, order)
        assert np.array_equal(en, want_en) and np.array_equal(fb, want_fb), (name, order)
        out, lst, off, ln = run_final(harness, pre, ust, order)
        assert np.array_equal(out, want["outcome"]), (name, order)
        assert np.array_equal(fb, want["first_bad"])
        assert np.array_equal(lst, want["accepted"]) and np.array_equal(off, 32 * lst.astype(np.uint64))
        assert (ln == 32).all()


def test_precedence_is_exhaustive_and_every_outcome_occurs():
    """The restatement itself: 128 combinations of the seven conditions, and each class of outcome among them."""
    txs = C.precedence_cases()
    assert len(txs) == 128 + 32                    # a bad signature AND a bad key come in both orders
    pre, _, fb = C.gate(txs, 1)
    assert set(pre.tolist()) == set(range(8))
    assert ((fb != C.NO_SIG) == np.isin(pre, (C.TX_INVALID, C.BAD_KEY))).all()
    # not validating: the signature conditions and the requirements decide nothing
    assert set(C.gate(txs, 0)[0].tolist()) == {C.SUCCESS, C.EMPTY, C.ID_MISMATCH, C.TIMESTAMP_INVALID}
    both, resident = C.conflict_cases()
    assert C.CONFLICT in C.notarise(both, 1, resident)["outcome"]


def test_null_prefilters(harness):
    """tx_pre and sig_pre are optional: without them only the bitmap and the device status decide."""
    txs = C.prefilter_cases()
    f = C.flatten(txs)
    plain = [dict(t, tx_pre=0, sigs=[(b, s, 0) for b, s, _ in t["sigs"]]) for t in txs]
    want = C.gate(plain, 1)
    for order in ORDERS:
        got = run_gate(harness, f, 1, order, with_pre=False)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_gather_is_the_sha256_byte_string(harness):
    """A leaf digest as the Merkle kernels keep it (big-endian state words) becomes the 32 bytes of hashlib's digest,
    for states that repeat leaves and skip leaves, in every lane order."""
    rng = np.random.default_rng(5)
    leaves = [bytes(rng.integers(0, 256, int(rng.integers(0, 80)), dtype=np.uint8)) for _ in range(70)]
    digs = np.array([np.frombuffer(hashlib.sha256(b).digest(), ">u4") for b in leaves]).astype(np.uint32)
    state_leaf = rng.integers(0, 70, 200).astype(np.uint32)
    for order in ORDERS:
        key = np.full((200, 32), 0xEE, np.uint8)
        harness.hnt_gather(200, _p(digs), _p(state_leaf), order, _p(key))
        assert all(key[i].tobytes() == hashlib.sha256(leaves[state_leaf[i]]).digest() for i in range(200))


def test_argument_checks_without_a_device():
    """cv_notarise_batch's checks run before any device work: ntx == 0 is CV_OK and touches nothing, a null context is
    CV_E_ARGS, so are malformed ranges and an input count above the leaf count."""
    from corda_amd import native
    lib = native.load()
    P = native._p
    nul = [None] * 11
    assert lib.cv_notarise_batch(None, None, None, 1, 0, None, 0, *nul, 0, 0, 0, *([None] * 19)) == 0
    z4, b64, b32 = np.zeros(4, np.uint32), np.zeros(64, np.uint8), np.zeros(32, np.uint8)
    off, ln = np.zeros(1, np.uint64), np.array([8], np.uint32)

    def call(txb, cnt, arena_bytes=8, outcome=b32, sig=b64):
        sc = [P(np.zeros(32, np.uint8)), P(np.zeros(32, np.uint8)), P(np.zeros(4, np.uint32)), P(np.zeros(4, np.uint32))]
        return lib.cv_notarise_batch(None, None, None, 0, 1, P(np.zeros(8, np.uint8)), arena_bytes, P(off), P(ln),
                                     P(np.array(txb, np.uint32)), P(np.array(cnt, np.uint32)), P(b32), P(z4), None, None,
                                     None, None, None, 0, 0, 0, *([None] * 10), P(outcome) if outcome is not None else None,
                                     None, P(sig), None, None, *sc)
    assert call([0, 1], [1]) == -3                     # everything in order but the context
    assert call([0, 1], [2]) == -3                     # more inputs than leaves
    assert call([1, 1], [0]) == -3                     # begin[0] != 0
    assert call([0, 1], [0], arena_bytes=7) == -3      # a leaf past the arena
    assert call([0, 1], [0], outcome=None) == -3
    assert lib.cv_notarise_batch(None, None, None, 0, 0xffffffff, None, 0, *nul, 0, 0, 0, *([None] * 19)) == -5


def test_sanitizers_standalone_program():
    """tests/notary_san.cpp (its own main: random batches against a sequential model) under ASan + UBSan, run as a
    subprocess: nothing is loaded into this process under a sanitizer."""
    exe = os.path.join(REPO, "tests", "_build", "notary_san")
    src = os.path.join(REPO, "tests", "notary_san.cpp")
    if _stale(exe, _deps(src, os.path.join(REPO, "tests", "notary_harness.cpp"))):
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
