"""The missing-signers core compiled for the CPU (corda_amd/csrc/cv_ck.h through tests/ck_harness.cpp) against
fulfilled_ref, the literal restatement of CompositeKey.isFulfilledBy in tests/ck_cases.py, exactly: every case with
wide_min 0, 1 and UINT32_MAX and the lanes of every phase — the narrow path's transactions, the wide path's lanes and
waves — in ascending, descending and one shuffled order; the oracle against the mirror; the mirror's flattener against
the cases'; the Abyte rule; the C-ABI's argument checks that need no device; and the same core under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/ck_san.cpp).  No GPU.

Reference: SignedTransaction.kt:58-72,89-93, CompositeKey.kt:22-108, CompositeKeyTests.kt:22-49, TransactionTests.kt:25-58.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ck_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
ORDERS = (0, 1, 2)              # the harness's lane orders: ascending, descending, shuffled
ARRAYS = ("kind", "leaf_key", "threshold", "child_begin", "child", "weight", "req_begin", "tx_req_begin", "sig_key",
          "tx_sig_begin", "req_allowed", "bitmap")


def _deps(*srcs):
    return list(srcs) + [os.path.join(REPO, "corda_amd", "csrc", "cv_ck.h")]


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def harness():
    """tests/ck_harness.cpp built as tests/test_uniq_cpu.py builds its harness."""
    lib = os.path.join(REPO, "tests", "_build", "libcvck.so")
    src = os.path.join(REPO, "tests", "ck_harness.cpp")
    if _stale(lib, _deps(src)):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-O2", "-std=c++17", "-fPIC",
                        "-shared", src, "-o", lib], check=True)
    h = ctypes.CDLL(lib)
    h.hck_run.restype = ctypes.c_int64
    h.hck_run.argtypes = [ctypes.c_uint32] * 5 + [ctypes.c_void_p] * 12 + [ctypes.c_uint32, ctypes.c_int] + [ctypes.c_void_p] * 2
    h.hck_workspace.restype = ctypes.c_uint64
    h.hck_workspace.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    h.hck_tile.restype = ctypes.c_uint32
    h.hck_wide_default.restype = ctypes.c_uint32
    return h


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _pad(a):
    """An array the harness can take a pointer of (an empty one becomes one zero row)."""
    return a if a is None or a.size else np.zeros((1,) + a.shape[1:], a.dtype)


def run(h, f, wide_min, order, fill=0xEE):
    """(req_missing, tx_status, transactions the wide path decided) of the flat arrays f."""
    ntx, nreq, nnodes = f["tx_req_begin"].size - 1, f["req_begin"].size - 1, f["child_begin"].size - 1
    nchild, nsig = f["child"].size, f["sig_key"].shape[0]
    rm, st = np.full(max(nreq, 1), fill, np.uint8), np.full(max(ntx, 1), fill, np.uint8)
    a = [_pad(f[k]) for k in ARRAYS]
    wide = h.hck_run(ntx, nreq, nnodes, nchild, nsig, *[_p(x) for x in a], wide_min, order, _p(rm), _p(st))
    assert wide >= 0
    return rm[:nreq], st[:ntx], int(wide)


@pytest.fixture(scope="module")
def built():
    return {name: C.build(make()) for name, make in C.CASES.items()}


def test_tile_matches_the_header(harness):
    assert harness.hck_tile() == C.TILE and harness.hck_wide_default() == 4096


def test_oracle_equals_the_mirror_where_nothing_overflows():
    """fulfilled_ref == crypto.CompositeKey.is_fulfilled_by on every case but the overflow one, where the mirror's
    unbounded sum says fulfilled and Kotlin's Int says missing."""
    for name, make in C.CASES.items():
        case = make()
        assert C.mirror_agrees(case) != case.overflows, name
    big = C.overflow().txs[0]
    assert not C.fulfilled_ref(big.must_sign[0], set(big.signers)) and big.must_sign[0].is_fulfilled_by(set(big.signers))


@pytest.mark.parametrize("wide_min", C.WIDE_MINS)
@pytest.mark.parametrize("name", list(C.CASES))
def test_cases_in_every_lane_order(harness, built, name, wide_min):
    f, want_missing, want_status = built[name]
    before = {k: None if f[k] is None else f[k].copy() for k in ARRAYS}
    wides = []
    for order in ORDERS:
        for fill in (0xEE, 0x11):
            rm, st, wide = run(harness, f, wide_min, order, fill)
            assert rm.tolist() == want_missing.tolist(), (name, wide_min, order)
            assert st.tolist() == want_status.tolist(), (name, wide_min, order)
        wides.append(wide)
    for k in ARRAYS:                                             # inputs are only read
        assert before[k] is None or np.array_equal(before[k], f[k])
    ntx = want_status.size
    assert len(set(wides)) == 1
    assert wides[0] == {0: wides[0], 1: ntx, 0xFFFFFFFF: 0}[wide_min]
    if wide_min == 0:
        # the default threshold takes the large shapes to the wave path and nothing else
        assert wides[0] == {"wide_shapes": ntx, "outlier_300x300": 1}.get(name, 0)


def test_wide_min_threshold(harness):
    """A transaction goes to the wave path iff max(nodes, 1) x max(signers, 1) >= wide_min: 3 nodes x 5 signers at 15
    and 16, a transaction without nodes and one without signers at 1 and 2; the results are the same either side."""
    x, y = C.leaf("thr", 0), C.leaf("thr", 1)
    signers = [C.key("thr", i) for i in range(5)]
    case = C.Case([C.Tx([C.node(1, [x, y])], signers), C.Tx([], signers[:1]), C.Tx([x], [])])
    f, want_missing, want_status = C.build(case)
    for wide_min, wide in ((15, 1), (16, 0), (1, 3), (2, 1), (5, 1), (0xFFFFFFFE, 0)):
        for order in ORDERS:
            rm, st, got = run(harness, f, wide_min, order)
            assert (rm.tolist(), st.tolist(), got) == (want_missing.tolist(), want_status.tolist(), wide), (wide_min, order)


def test_mirror_flattener_equals_the_cases(built):
    """transactions.flatten_must_sign (what the mirror hands the device) gives the arrays the cases' flattener gives."""
    from corda_amd.crypto import DigitalSignature
    from corda_amd.transactions import SecureHash, SignedTransaction, WireTransaction, flatten_must_sign
    for name in ("composite_key_tests", "transaction_tests", "weights_thresholds", "structure", "req_allowed", "batch_65"):
        case = C.CASES[name]()
        txs = [tx for tx in case.txs if tx.signers]                 # a SignedTransaction has a signature
        stxs = [SignedTransaction(WireTransaction(must_sign=tx.must_sign),
                                  [DigitalSignature.WithKey(k, bytes(64)) for k in tx.signers], SecureHash(bytes(32)))
                for tx in txs]
        want = C.flatten(txs)
        allowed = [r for tx in txs for r in tx.allowed]
        got = flatten_must_sign(stxs, allowed)
        for k in want:
            if k == "req_allowed" and any(set(tx.allowed) != set(allowed) for tx in txs):
                continue                                           # the cases allow per transaction, the mirror per batch
            assert np.array_equal(want[k], got[k]) and want[k].dtype == got[k].dtype, (name, k)


def test_abyte_rule(harness):
    """The call compares the 32 bytes it is given: the wire key ed ff .. ff 7f (y = p) against a Leaf of 32 zero bytes
    is missing as given, and fulfilled once both sides go through getAbyte() (oracle/ed25519_ref.py abyte_of)."""
    from ed25519_ref import abyte_of
    from corda_amd.crypto import EdDSAPublicKey
    wire = bytes([0xED] + [0xFF] * 30 + [0x7F])
    assert abyte_of(wire) == bytes(32) and abyte_of(bytes([0xEE] + [0xFF] * 30 + [0x7F])) == bytes([1] + [0] * 31)
    as_given = C.Case([C.Tx([C.Leaf(EdDSAPublicKey(bytes(32)))], [EdDSAPublicKey(wire)])])
    canonical = C.Case([C.Tx([C.Leaf(EdDSAPublicKey(abyte_of(bytes(32))))], [EdDSAPublicKey(abyte_of(wire))])])
    for wide_min in C.WIDE_MINS:
        f, _, _ = C.build(as_given)
        assert [x.tolist() for x in run(harness, f, wide_min, 0)[:2]] == [[C.MISSING], [C.VS_MISSING]]
        f, _, _ = C.build(canonical)
        assert [x.tolist() for x in run(harness, f, wide_min, 0)[:2]] == [[C.FULFILLED], [C.VS_OK]]


def test_workspace_size(harness):
    from corda_amd import native
    up16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    for ntx, nnodes in ((0, 0), (1, 1), (1, 17), (255, 1000), (4096, 3 * 4096 + 1), (1 << 20, 5 << 20)):
        want = 16 + up16(4 * ntx) + up16(nnodes)                  # the counter | the list | the flags
        assert native.missing_signers_workspace(ntx, nnodes) == want == harness.hck_workspace(ntx, nnodes)


def test_argument_checks_without_a_device():
    """The C-ABI's checks that run before any device call: ntx == 0 is CV_OK and touches nothing, counts past 32 bits
    CV_E_TOO_LARGE, malformed ranges and missing arrays CV_E_ARGS, and last of all the null context CV_E_ARGS."""
    from corda_amd import native
    lib = native.load()
    OK, ARGS, TOO_LARGE = 0, -3, -5
    f, _, _ = C.build(C.transaction_tests())
    ntx, nreq, nnodes = f["tx_req_begin"].size - 1, f["req_begin"].size - 1, f["child_begin"].size - 1
    rm, st = np.full(nreq, 9, np.uint8), np.full(ntx, 9, np.uint8)
    names = ARRAYS[:10]

    def call(counts=None, rm_=rm, st_=st, **repl):
        a = {k: _pad(f[k]) for k in names}
        a.update(repl)
        c = counts or (ntx, nreq, nnodes, f["child"].size, f["sig_key"].shape[0])
        return lib.cv_missing_signers(None, *c, *[native._p(a[k]) for k in names], None, None, 0, native._p(rm_), native._p(st_))

    u32 = lambda *v: np.array(v, np.uint32)  # noqa: E731
    assert call() == ARGS                                                           # well formed: the null context
    assert call(counts=(0, 0, 0, 0, 0)) == OK
    assert lib.cv_missing_signers(None, 0, 0, 0, 0, 0, *[None] * 12, 0, None, None) == OK
    for k in ("req_begin", "tx_req_begin", "tx_sig_begin"):
        bad = f[k].copy()
        bad[0] = 1
        assert call(**{k: bad}) == ARGS, k                                          # begin[0] != 0
        bad = f[k].copy()
        bad[-1] += 1
        assert call(**{k: bad}) == ARGS, k                                          # the last entry is not the count
        bad = f[k].copy()
        bad[1], bad[2] = bad[2] + 1, bad[1]
        assert call(**{k: bad}) == ARGS, k                                          # not monotone
        assert call(**{k: None}) == ARGS, k
    for bad in (np.concatenate([u32(1), f["child_begin"][1:]]), np.concatenate([f["child_begin"][:-1], u32(1)])):
        assert call(child_begin=bad) == ARGS                                        # child_begin's two ends
    for k in ("kind", "leaf_key", "threshold", "child_begin", "sig_key"):
        assert call(**{k: None}) == ARGS, k
    g, _, _ = C.build(C.weights_thresholds())                                       # a batch with child entries
    gc = (g["tx_req_begin"].size - 1, g["req_begin"].size - 1, g["child_begin"].size - 1, g["child"].size, g["sig_key"].shape[0])
    grm, gst = np.full(gc[1], 9, np.uint8), np.full(gc[0], 9, np.uint8)
    for k in (None, "child", "weight"):
        a = [None if n == k else native._p(_pad(g[n])) for n in names]
        assert lib.cv_missing_signers(None, *gc, *a, None, None, 0, native._p(grm), native._p(gst)) == ARGS, k
    assert call(rm_=None) == ARGS and call(st_=None) == ARGS
    for i in range(5):
        c = [ntx, nreq, nnodes, f["child"].size, f["sig_key"].shape[0]]
        c[i] = 0xFFFFFFFF
        assert call(counts=tuple(c)) == TOO_LARGE, i
    # the device form: its context first, then an empty call, then the counts
    dev = lambda ctx, ntx_: lib.cv_missing_signers_device(ctx, 0, ntx_, 0, 0, 0, 0, *[None] * 12, 0, None, None, None, None)  # noqa: E731
    assert dev(None, 0) == ARGS and dev(None, 1) == ARGS
    assert rm.tolist() == [9] * nreq and st.tolist() == [9] * ntx and (grm == 9).all() and (gst == 9).all()


def test_sanitizers_standalone_program():
    """tests/ck_san.cpp (its own main: random forests, DAGs and hostile child arrays against a sequential
    restatement, and the wide shapes) under ASan + UBSan, run as a subprocess: nothing is loaded into this process
    under a sanitizer."""
    exe = os.path.join(REPO, "tests", "_build", "ck_san")
    src = os.path.join(REPO, "tests", "ck_san.cpp")
    if _stale(exe, _deps(src, os.path.join(REPO, "tests", "ck_harness.cpp"))):
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
