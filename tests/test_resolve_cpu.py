"""The graph half of cv_resolve_batch compiled for the CPU (corda_amd/csrc/cv_resolve.h through
tests/resolve_harness.cpp) against the restatement of ResolveTransactionsFlow.call in tests/resolve_cases.py: the
join table's insert, its probe and the gate with the lanes of every step run in ascending, descending and one shuffled
order, then the library's own host order and walk; a table forced small so that probes collide, chain and wrap; the
duplicate word under every winner; the C-ABI's argument checks that need no device; and the same code under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program (tests/resolve_san.cpp).  No GPU.

Reference: ResolveTransactionsFlow.kt:37-67,96-111,170; SignedTransaction.kt:34-38,58-93,134; ServiceHub.kt:46-49.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import resolve_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
ORDERS = (0, 1, 2)              # the harness's lane orders: ascending, descending, shuffled
CSRC = os.path.join(REPO, "corda_amd", "csrc")


def _deps(*srcs):
    return list(srcs) + [os.path.join(CSRC, h) for h in ("cv_resolve.h", "cv_notary.h", "cv_uniq.h", "cv_table.h")]


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def harness():
    """tests/resolve_harness.cpp built as tests/test_notary_cpu.py builds its harness."""
    lib = os.path.join(REPO, "tests", "_build", "libcvresolve.so")
    src = os.path.join(REPO, "tests", "resolve_harness.cpp")
    if _stale(lib, _deps(src)):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-O2", "-std=c++17", "-fPIC",
                        "-shared", src, "-o", lib], check=True)
    h = ctypes.CDLL(lib)
    vp = ctypes.c_void_p
    h.hrs_run.argtypes = [ctypes.c_uint32, ctypes.c_uint32] + [vp] * 12 + [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int] + [vp] * 7
    h.hrs_run.restype = ctypes.c_int
    h.hrs_slots.argtypes = [ctypes.c_uint32]
    h.hrs_slots.restype = ctypes.c_uint32
    return h


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run(h, f, order, seed=0x9e3779b97f4a7c15, slots=0):
    """The three lane steps in `order`, then the host order and walk -> the outputs by name, poisoned before."""
    n, ni = f["ntx"], len(f["input_index"])
    out = dict(outcome=np.full(n, 0xEE, np.uint8), first_bad=np.full(n, 0xEEEEEEEE, np.uint32),
               bad_input=np.full(n, 0xEEEEEEEE, np.uint32), input_dep=np.full(ni, 0xEEEEEEEE, np.uint32),
               input_status=np.full(ni, 0xEE, np.uint8), order=np.full(n, 0xEEEEEEEE, np.uint32),
               graph=np.full(len(C.G_WORDS), 0xEEEEEEEE, np.uint32))
    rc = h.hrs_run(n, ni, _p(f["claimed"]), _p(f["tx_input_begin"]), _p(f["input_txhash"]), _p(f["input_index"]),
                   _p(f["tx_output_count"]), _p(f["mstatus"]), _p(f["id"]), _p(f["tx_sig_begin"]), _p(f["bitmap"]),
                   _p(f["sig_status"]), _p(f["sig_pre"]), _p(f["ck"]), seed, slots, order,
                   *[_p(out[k]) for k in ("outcome", "first_bad", "bad_input", "input_dep", "input_status", "order", "graph")])
    assert rc == 0, rc
    return out


@pytest.fixture(scope="module")
def reference():
    """resolve_ref of every case, computed once."""
    memo = {}

    def get(name, n):
        if (name, n) not in memo:
            txs = C.concrete(C.CASES[name](n))
            memo[name, n] = (C.flatten(txs), C.resolve_ref(txs))
        return memo[name, n]
    return get


@pytest.mark.parametrize("name,n", C.all_cases())
def test_cases_in_every_lane_order(harness, reference, name, n):
    """Every output equals the restatement's, whichever order the lanes run in."""
    f, want = reference(name, n)
    for order in ORDERS:
        C.same(run(harness, f, order), want, (name, n, order))


def test_every_class_and_status_occurs(reference):
    """The cases themselves: every outcome, every stop class and every graph status is met somewhere."""
    outcomes, stops, statuses = set(), set(), set()
    for name, n in C.all_cases((65,)) + [("fan_in", 1025), ("fan_out", 5000)]:
        _, want = reference(name, n)
        outcomes |= set(want["outcome"].tolist())
        stops.add(int(want["graph"][3]))
        statuses.add(int(want["graph"][0]))
    assert outcomes == {C.OK, C.EMPTY, C.ID_MISMATCH, C.TX_INVALID, C.BAD_KEY, C.SIGNATURES_MISSING, C.MALFORMED, C.BAD_INPUT}
    assert stops == {C.NONE, C.TX_INVALID, C.BAD_KEY, C.SIGNATURES_MISSING, C.MALFORMED, C.BAD_INPUT, C.UNRESOLVED}
    assert statuses == {C.G_OK, C.G_BAD_ID, C.G_DUPLICATE_ID}


def test_precedence_of_the_pairs(reference):
    """What the pairs pin: an unresolved input is met before an out-of-range one behind it and after one before it; a
    signature class wins over the inputs; an id mismatch fails the flow before anything."""
    g = lambda name: dict(zip(C.G_WORDS, reference(name, 2)[1]["graph"].tolist()))
    assert (g("unresolved_then_out_of_range")["stop_class"], g("unresolved_then_out_of_range")["stop_input"]) == (C.UNRESOLVED, 0)
    assert (g("pair_bad_input_unresolved")["stop_class"], g("pair_bad_input_unresolved")["stop_input"]) == (C.BAD_INPUT, 0)
    assert g("pair_bad_sig_unresolved")["stop_class"] == C.TX_INVALID
    assert g("pair_bad_sig_missing")["stop_class"] == C.TX_INVALID
    assert g("pair_missing_bad_input")["stop_class"] == C.SIGNATURES_MISSING
    assert g("pair_id_mismatch_bad_sig")["status"] == C.G_BAD_ID


@pytest.mark.parametrize("name,n", [("chain", 62), ("chain_reversed", 125), ("fan_in", 1020), ("duplicate_id", 62),
                                    ("cycle_off_chain", 63)])
def test_full_table_collides_chains_and_wraps(harness, reference, name, n):
    """A table of the smallest power of two that holds the batch and leaves a slot empty (an outside input's probe
    ends at an empty slot), so nearly full: the results do not change with the seed or the lane order, probes run
    longer than one slot and pass the last slot."""
    f, want = reference(name, n)
    slots = harness.hrs_slots((n + 2) // 2)
    assert n < slots <= n + 4
    wraps = 0
    for seed in (1, 2, 0xdeadbeefcafef00d):
        for order in ORDERS:
            got = run(harness, f, order, seed=seed, slots=slots)
            C.same(got, want, (name, n, seed, order))
            assert got["graph"][7] > 2
            wraps += int(got["graph"][8])
    assert wraps > 0


def test_which_under_every_winner(harness, reference):
    """duplicate_id holds one id at indices 1, 2, 3 and another at 4, 5: whichever of them claims the slot first (lane
    orders 3 + k start at lane k), WHICH is 1 and an input that names the id resolves to 1."""
    f, want = reference("duplicate_id", 64)
    assert want["graph"][0] == C.G_DUPLICATE_ID and want["graph"][1] == 1 and want["input_dep"][0] == 1
    for first in range(6):
        C.same(run(harness, f, 3 + first), want, first)
    # the other id alone: its smallest index
    txs = C.concrete([C.spec([("e", 0)]), C.spec([("f", 0)]), C.spec([("e", 0)], same_as=1)])
    for order in (0, 1, 2, 3, 4, 5):
        got = run(harness, C.flatten(txs), order)
        assert got["graph"][0] == C.G_DUPLICATE_ID and got["graph"][1] == 1


def test_order_is_a_topological_order_on_random_acyclic_graphs(harness):
    """The restatement itself, and the library's host code against it: on random acyclic graphs in random download
    orders, order is a permutation in which every dependency of the batch stands before its dependents, and nothing
    stops the walk."""
    rng = np.random.default_rng(11)
    for n in (1, 2, 7, 64, 300, 1025):
        for _ in range(4):
            specs = C.random_acyclic(rng, n)
            txs = C.concrete(specs)
            want = C.resolve_ref(txs)
            order = want["order"].tolist()
            pos = {t: p for p, t in enumerate(order)}
            assert sorted(order) == list(range(n)) and want["graph"][2] == n and want["graph"][3] == C.NONE
            for t, s in enumerate(specs):
                assert all(pos[r] < pos[t] for r, _ in s["inputs"] if isinstance(r, int))
            C.same(run(harness, C.flatten(txs), 2), want, n)


def test_wrap_seed_for_the_gpu_run(harness):
    """resolve_cases.WRAP_SEED, the seed tests/test_gpu_resolve.py passes for chain(65) as real() builds it (the ids
    hashed on the host here), makes a probe of the library-sized table pass its last slot."""
    specs = C.CASES["chain"](65)
    txs = C.concrete(specs, C.real_leaves(specs)[2])
    got = run(harness, C.flatten(txs), 0, seed=C.WRAP_SEED)
    C.same(got, C.resolve_ref(txs))
    assert got["graph"][8] > 0


def test_argument_checks_without_a_device():
    """cv_resolve_batch's checks run before any device work: ntx == 0 is CV_OK and touches nothing, the limits are
    CV_E_TOO_LARGE, malformed ranges, a leaf past the arena, a missing array and a null context are CV_E_ARGS."""
    from corda_amd import native
    lib = native.load()
    P = native._p
    u32 = lambda *a: np.array(a, np.uint32)

    def call(ntx=1, txb=(0, 1), arena_bytes=8, tsb=(0, 1), nreq=0, trb=(0, 0), rb=(0,), ninputs=1, tib=(0, 1),
             outcome=True, input_dep=True, nnodes=0, nchild=0, leaf_len=8):
        keep = [np.zeros(8, np.uint8), np.zeros(1, np.uint64), u32(leaf_len), u32(*txb), np.zeros(32, np.uint8),
                np.zeros(32, np.uint8), np.zeros(64, np.uint8), u32(*tsb), u32(*rb), u32(*trb), np.zeros(32, np.uint8),
                u32(*tib), np.zeros(32, np.uint8), u32(0), u32(1)]
        arena, off, ln, txb_, claimed, pk, sig, tsb_, rb_, trb_, skey, tib_, txhash, index, nout = keep
        outs = [np.zeros(64, np.uint8) for _ in range(9)]
        o = [P(a) for a in outs]
        if not outcome:
            o[0] = None
        if not input_dep:
            o[4] = None
        return lib.cv_resolve_batch(None, ntx, P(arena), arena_bytes, P(off), P(ln), P(txb_), P(claimed), P(pk), P(sig),
                                    P(tsb_), None, nreq, nnodes, nchild, None, None, None, None, None, None, P(rb_), P(trb_),
                                    P(skey), ninputs, P(tib_), P(txhash), P(index), P(nout), 0, *o)
    assert lib.cv_resolve_batch(None, 0, None, 0, *([None] * 8), 0, 0, 0, *([None] * 9), 0, *([None] * 4), 0,
                                *([None] * 9)) == 0
    assert call() == -3                                # everything in order but the context
    assert call(txb=(1, 1)) == -3                      # begin[0] != 0
    assert call(tsb=(1, 0)) == -3                      # not monotone
    assert call(tib=(0, 2)) == -3                      # the last entry is not the count
    assert call(trb=(0, 1)) == -3
    assert call(arena_bytes=7) == -3                   # a leaf past the arena
    assert call(leaf_len=0xffffffff) == -3
    assert call(outcome=False) == -3
    assert call(input_dep=False) == -3                 # an array that a non-zero count needs
    assert call(nnodes=1) == -3
    assert call(nchild=1) == -3
    assert call(ninputs=0, tib=(0, 0), input_dep=False) == -3      # ninputs == 0 is legal: only the context is missing
    assert call(ntx=0xffffffff) == -5
    assert call(ntx=(1 << 30) + 1) == -5
    assert call(ninputs=(1 << 30) + 1) == -5
    assert call(nreq=0xffffffff) == -5


def test_sanitizers_standalone_program():
    """tests/resolve_san.cpp (its own main: random graphs against a sequential model, a chain of 2^20) under ASan +
    UBSan, run as a subprocess: nothing is loaded into this process under a sanitizer."""
    exe = os.path.join(REPO, "tests", "_build", "resolve_san")
    src = os.path.join(REPO, "tests", "resolve_san.cpp")
    if _stale(exe, _deps(src, os.path.join(REPO, "tests", "resolve_harness.cpp"))):
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
