"""PartialMerkleTree.build on the device code compiled for the CPU (corda_amd/csrc/cv_pmt_build.h through
tests/pmt_build_harness.cpp) against the oracle (oracle/merkle_ref.py: get_merkle_tree, build_partial, flatten), byte
for byte; the bound; the C-ABI's argument checks that need no device; and the same core under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/pmt_build_san.cpp).  No GPU.

Reference: PartialMerkleTree.kt:69-111, MerkleTransaction.kt:49-101, PartialMerkleTreeTest.kt:88-120.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import merkle_ref as M
import pmt_build_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _deps(*srcs):
    csrc = os.path.join(REPO, "corda_amd", "csrc")
    return list(srcs) + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def harness():
    """tests/pmt_build_harness.cpp built as tests/test_sign_keyed_cpu.py builds sign_harness.cpp."""
    lib = os.path.join(REPO, "tests", "_build", "libcvpmtb.so")
    src = os.path.join(REPO, "tests", "pmt_build_harness.cpp")
    if _stale(lib, _deps(src)):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-DCV_BOUNDS_CHECK", "-fPIC", "-shared", src,
                        "-o", lib], check=True)
    h = ctypes.CDLL(lib)
    h.cvb_bound.restype = ctypes.c_uint64
    h.cvb_pyramid.restype = ctypes.c_uint64
    h.cvb_build.restype = ctypes.c_uint32
    return h


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _build(h, b, use_keep):
    """The batch through the harness -> (kind, left, right, node_hash, tree_begin, ids, status), cut to the nodes."""
    ntx = b["ntx"]
    cap = sum(int(h.cvb_bound(int(n))) for n in np.diff(b["txb"].astype(np.int64)))
    m = max(cap, 1)
    kind, left, right = np.full(m, 0xEE, np.uint8), np.full(m, 0xEEEEEEEE, np.uint32), np.full(m, 0xEEEEEEEE, np.uint32)
    node_hash = np.full((m, 32), 0xEE, np.uint8)
    tb, ids, st = np.zeros(ntx + 1, np.uint32), np.zeros((ntx, 32), np.uint8), np.zeros(ntx, np.uint8)
    lh = b["leaf_hash"] if b["leaf_hash"].size else np.zeros((1, 32), np.uint8)
    inc = b["include"] if b["include"].size else np.zeros((1, 32), np.uint8)
    nn = h.cvb_build(ntx, _p(lh), _p(b["txb"]), None if use_keep else _p(inc), None if use_keep else _p(b["inc_begin"]),
                     _p(b["keep"] if b["keep"].size else np.zeros(1, np.uint8)) if use_keep else None, _p(kind), _p(left),
                     _p(right), _p(node_hash), _p(tb), _p(ids), _p(st))
    assert nn <= cap
    return kind[:nn], left[:nn], right[:nn], node_hash[:nn], tb, ids, st


def _assert_equal(got, b):
    for name, a in zip(("kind", "left", "right", "node_hash", "tree_begin", "ids", "status"), got):
        assert a.shape == b[name].shape and np.array_equal(a, b[name]), name


def test_exhaustive_both_sources(harness):
    """Every include subset of 0..8 leaves (511 transactions), as an explicit digest list and as a keep mask."""
    b = C.exhaustive_batch()
    assert b["ntx"] == 511 and (b["status"] == C.EMPTY).sum() == 1 and (b["status"] == C.OK).sum() == 510
    _assert_equal(_build(harness, b, use_keep=False), b)
    _assert_equal(_build(harness, b, use_keep=True), b)


def test_random_trees(harness):
    """300 trees of 1..70 leaves with repeated leaves, absent and repeated includes, shuffled include order."""
    b = C.random_batch()
    assert b["ntx"] == 300 and (b["status"] == C.NOT_IN_TREE).sum() >= 40 and (b["status"] == C.OK).sum() >= 150
    _assert_equal(_build(harness, b, use_keep=False), b)


def test_random_trees_keep_mask(harness):
    """The same trees with a keep mask: a kept leaf that another leaf repeats fails as in the reference."""
    b = C.random_keep_batch()
    assert (b["status"] == C.NOT_IN_TREE).sum() >= 5 and (b["status"] == C.OK).sum() >= 200
    _assert_equal(_build(harness, b, use_keep=True), b)


def test_reference_scenarios(harness):
    h6 = C.hashed_abcdef()
    sc = C.reference_scenarios()
    assert len(sc) == 6
    b = C.batch_of([(lv, inc, None) for _, lv, inc, _ in sc] + [([h6[0], h6[0]], [h6[0], h6[0]], None)])
    assert b["status"].tolist() == [st for *_, st in sc] + [C.OK]          # two equal leaves, both listed: succeeds
    assert b["ids"][0].tobytes().hex().upper() == "F6D8FB3720114F8D040D64F633B0D9178EB09A55AA7D62FAE1A070D1BF561051"
    got = _build(harness, b, use_keep=False)
    _assert_equal(got, b)
    assert got[4][2] - got[4][1] == 1 and got[0][got[4][1]] == M.LEAF              # no include: one Leaf(root)
    assert got[3][got[4][1]].tobytes() == b["ids"][1].tobytes()
    # 'aaa' with the first leaf kept: 3 leaves carry the kept hash against a list of 1
    aaa = C.batch_of([([h6[0]] * 3, [h6[0]], [1, 0, 0])])
    assert aaa["status"].tolist() == [C.NOT_IN_TREE]
    _assert_equal(_build(harness, aaa, use_keep=True), aaa)


@pytest.mark.parametrize("name", ["exhaustive", "random"])
def test_round_trip_through_verify(harness, name):
    """Each built tree passes the host cv_pmt_verify with the built root and the include list; the root is the one
    cv_merkle_root_inplace gives."""
    b = C.exhaustive_batch() if name == "exhaustive" else C.random_batch()
    kind, left, right, node_hash, tb, ids, st = _build(harness, b, use_keep=False)
    inc = b["include"] if b["include"].size else np.zeros((1, 32), np.uint8)
    root = np.zeros(32, np.uint8)
    n_ok = n_bad = 0
    for t in range(b["ntx"]):
        lb, le = int(b["txb"][t]), int(b["txb"][t + 1])
        if le > lb:
            leaves = np.ascontiguousarray(b["leaf_hash"][lb:le])
            assert harness.cvb_root(le - lb, _p(leaves), _p(root)) == 1 and np.array_equal(root, ids[t]), t
        if st[t] != C.OK:
            assert tb[t + 1] == tb[t]
            continue
        n_ok += 1
        r = harness.cvb_verify(int(tb[t]), int(tb[t + 1]), _p(kind), _p(left), _p(right), _p(node_hash),
                               _p(np.ascontiguousarray(ids[t])), _p(inc), int(b["inc_begin"][t]), int(b["inc_begin"][t + 1]))
        # 1, except where the reference's own count rule lets a build through whose list is not the included leaves
        # (a leaf carried twice, listed once beside an absent hash: 2 used against 2 listed) — there the oracle's
        # verify says 0 as well
        lo, hi = int(b["inc_begin"][t]), int(b["inc_begin"][t + 1])
        eb, ee = int(b["tree_begin"][t]), int(b["tree_begin"][t + 1])
        included = sorted(b["node_hash"][k].tobytes() for k in range(eb, ee) if b["kind"][k] == M.INCLUDED)
        want = 1 if included == sorted(inc[j].tobytes() for j in range(lo, hi)) else 0
        assert r == want, (t, r)
        n_bad += 1 - want
    assert n_ok == (b["status"] == C.OK).sum() > 100
    assert n_bad == 0 if name == "exhaustive" else n_bad * 20 < n_ok


def _all_included_count(n):
    leaves = [bytes([i % 256, i // 256]) + bytes(30) for i in range(n)]
    return len(M.flatten(M.build_partial(M.get_merkle_tree(leaves), leaves))[0])


def test_bound(harness):
    """cv_partial_merkle_build_bound = the node count with every leaf included, L = 1..70 and 1,025; 13 and 141 for
    L = 5 and 65; the library's host function agrees with the device header's."""
    from corda_amd import native
    want = {n: _all_included_count(n) for n in list(range(1, 71)) + [1025]}
    assert want[5] == 13 and want[65] == 141
    for n, w in want.items():
        assert harness.cvb_bound(n) == w, n
        assert native.partial_merkle_build_bound(np.array([0, n], np.uint32)) == w, n
    assert harness.cvb_bound(0) == 0 and harness.cvb_pyramid(0) == 0 and harness.cvb_pyramid(5) == 11
    sizes = list(want)
    assert native.partial_merkle_build_bound(np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)) == sum(want.values())
    assert native.partial_merkle_build_bound(np.array([0], np.uint32)) == 0


def test_argument_checks_without_a_device():
    """The checks that run before any device call, with a null context: an empty batch is CV_OK and touches
    nothing, sizes past 32 bits are CV_E_TOO_LARGE, malformed ranges and missing arrays CV_E_ARGS — and a well-formed
    call is CV_E_ARGS for the null context, last."""
    from corda_amd import native
    lib = native.load()
    OK, ARGS, TOO_LARGE = 0, -3, -5
    u32 = lambda *v: np.array(v, np.uint32)  # noqa: E731
    leaf = np.zeros((4, 32), np.uint8)
    inc = np.zeros((2, 32), np.uint8)
    kind, left, right, hashes = np.zeros(16, np.uint8), np.zeros(16, np.uint32), np.zeros(16, np.uint32), np.zeros((16, 32), np.uint8)
    tb, ids, st = np.full(3, 7, np.uint32), np.zeros((2, 32), np.uint8), np.full(2, 9, np.uint8)
    nn = ctypes.c_size_t(77)

    def build(ntx, lh, txb, ic, ib, cap=16, kd=kind, tbo=tb, sto=st, nno=ctypes.byref(nn)):
        return lib.cv_partial_merkle_build(None, ntx, _p(lh), _p(txb), _p(ic), _p(ib), cap, _p(kd), _p(left), _p(right),
                                           _p(hashes), _p(tbo), _p(ids), _p(sto), nno)

    def filtered(ntx, txb, keep, off=np.zeros(4, np.uint64), ln=np.zeros(4, np.uint32)):
        return lib.cv_filtered_build(None, ntx, _p(np.zeros(16, np.uint8)), 16, _p(off), _p(ln), _p(txb), _p(keep), 16,
                                     _p(kind), _p(left), _p(right), _p(hashes), _p(tb), _p(ids), _p(st), ctypes.byref(nn))

    assert build(0, None, None, None, None, 0, None, None, None, None) == OK
    assert filtered(0, None, None, None, None) == OK
    assert build(2, leaf, u32(0, 2, 4), inc, u32(0, 1, 2)) == ARGS                      # well formed: the null context
    assert build(2, leaf, u32(1, 2, 4), inc, u32(0, 1, 2)) == ARGS                      # begin[0] != 0
    assert build(2, leaf, u32(0, 3, 2), inc, u32(0, 1, 2)) == ARGS                      # not monotone
    assert build(2, leaf, u32(0, 2, 4), inc, u32(0, 2, 1)) == ARGS
    assert build(2, None, u32(0, 2, 4), inc, u32(0, 1, 2)) == ARGS                      # leaves without hashes
    assert build(2, leaf, u32(0, 2, 4), None, u32(0, 1, 2)) == ARGS
    assert build(2, leaf, u32(0, 2, 4), inc, None) == ARGS
    assert build(2, leaf, u32(0, 2, 4), inc, u32(0, 1, 2), kd=None) == ARGS             # capacity without arrays
    assert build(2, leaf, u32(0, 2, 4), inc, u32(0, 1, 2), tbo=None) == ARGS
    assert build(2, leaf, u32(0, 2, 4), inc, u32(0, 1, 2), sto=None) == ARGS
    assert build(2, leaf, u32(0, 2, 4), inc, u32(0, 1, 2), nno=None) == ARGS
    # one transaction of 2^31 leaves: its pyramid alone passes 0xfffffffe nodes (nothing is read: the checks come first)
    assert native.partial_merkle_build_bound(u32(0, 1 << 31)) == (1 << 32) - 1          # 2^31 + 2^30 + ... + 1
    assert build(1, leaf, u32(0, 1 << 31), inc, u32(0, 0)) == TOO_LARGE
    assert filtered(1, u32(0, 1 << 31), np.zeros(4, np.uint8)) == TOO_LARGE
    assert build(0xffffffff, leaf, u32(0), inc, u32(0)) == TOO_LARGE
    assert filtered(2, u32(0, 2, 4), None) == ARGS                                      # no keep mask
    assert filtered(2, u32(0, 2, 4), np.zeros(4, np.uint8), off=None) == ARGS
    assert filtered(2, u32(0, 3, 2), np.zeros(4, np.uint8)) == ARGS
    assert filtered(2, u32(0, 2, 4), np.zeros(4, np.uint8)) == ARGS                     # well formed: the null context
    assert nn.value == 77 and tb.tolist() == [7, 7, 7] and st.tolist() == [9, 9]       # nothing was written


def test_sanitizers_standalone_program():
    """tests/pmt_build_san.cpp (its own main; the exhaustive cases and their round trip) under ASan + UBSan, run as
    a subprocess: nothing is loaded into this process under a sanitizer."""
    exe = os.path.join(REPO, "tests", "_build", "pmt_build_san")
    src = os.path.join(REPO, "tests", "pmt_build_san.cpp")
    if _stale(exe, _deps(src, os.path.join(REPO, "tests", "pmt_build_harness.cpp"))):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-O1", "-g", "-std=c++17",
                        "-DCV_BOUNDS_CHECK", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                        "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer", src, "-o", exe,
                        "-fsanitize=address,undefined"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    for bad in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"):
        assert bad not in out, out[-4000:]
    assert r.stdout.split() == ["ok", "1022"]
