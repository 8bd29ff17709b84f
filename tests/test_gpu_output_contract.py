"""The output contract of the device-resident API (include/cordaverify.h): outputs may hold anything on entry, the
bits of the last bitmap word at and above n are written as zero, an empty transaction's id is 32 zero bytes,
nothing before or behind an output is written, inputs are read-only, and every pointer needs no more than the
alignment the header states.

Every output is carved from a poisoned, guard-banded device allocation (tests/guarded.py) at the minimum alignment
of the contract (the bitmap at 8 mod 16, status at an odd address, records at 16 mod 32).  Inputs are rows of
tests/golden/ed25519_corpus.npz, whose verdict and status columns are the reference (the CPU suite ties them to
oracle/ed25519_ref.py and the C oracle); signatures are compared with oracle/ed25519_ref.py, Merkle ids with the C
oracle.  Every comparison is equality of bytes.

Sizes: the smallest at which each kernel's indexing can go wrong — one record; the tri wave of 4 signatures
(3, 4, 5); CV_FIN_CHUNK = 8; the quad wave of 16; the bitmap word and throughput wave of 64; two words; CV_BLOCK =
256; the workspace granule of 512.  For each size two batches: one whose LAST record is accepted (a lane past n that
replays it and keeps its verdict sets a tail bit) and one whose last record is a CV_SIG_BAD_KEY row.
"""
import ctypes

import numpy as np
import pytest
import torch

import ed25519_ref as E
from corda_amd import native
from guarded import DEVICE_ALIGN as AL, Guarded, Options, corpus_rows as _rows, tail_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513]
# (CV_OPT_QUAD_MAX, CV_OPT_TRI_MAX), as test_lane_quad_and_tri_forms_agree forces the forms
FORMS = {"throughput": (0, 0), "quad": (1 << 22, 0), "tri": (1 << 22, 1 << 20)}
FILLS = (0x00, 0xFF)
LAST = ("accepted", "bad_key")


def _up(a) -> torch.Tensor:
    """A host array's bytes in a device tensor of its own (the allocator's alignment: 512 bytes)."""
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(DEV)


class _Batch:
    """The rows' records on the device, with a second copy to compare the inputs against after each call."""

    def __init__(self, corpus, arena_dev, rows):
        self.n = len(rows)
        self.verdict = corpus["verdict"][rows].astype(bool)
        self.status = corpus["status"][rows].astype(np.uint8)
        self.pk_rows = corpus["pk"][rows]
        self.t = {"pk": _up(self.pk_rows), "sig": _up(corpus["sig"][rows]), "arena": arena_dev[0],
                  "off": _up(corpus["off"][rows].astype(np.uint64)), "len": _up(corpus["len"][rows].astype(np.uint32))}
        self.orig = {k: (arena_dev[1] if k == "arena" else v.clone()) for k, v in self.t.items()}

    def add_keys(self):
        keys, inv = np.unique(self.pk_rows, axis=0, return_inverse=True)
        self.nkeys = len(keys)
        self.t["keys"] = _up(keys)
        self.t["key_index"] = _up(inv.reshape(-1).astype(np.uint32))
        for k in ("keys", "key_index"):
            self.orig[k] = self.t[k].clone()
        return self

    def p(self, name) -> int:
        return self.t[name].data_ptr()

    def assert_inputs_unchanged(self, what, names=("pk", "sig", "arena", "off", "len")):
        for k in names:
            assert torch.equal(self.t[k], self.orig[k]), (what, f"input {k} was written")


@pytest.fixture(scope="module")
def arena_dev(corpus):
    a = _up(corpus["arena"])
    return a, a.clone()


@pytest.fixture(scope="module")
def batches(corpus, arena_dev):
    """(n, last) -> the batch on the device, built once for the module and never written."""
    return {(n, last): _Batch(corpus, arena_dev, _rows(corpus, n, last)).add_keys() for n in SIZES for last in LAST}


def _outputs(n, with_status, fill):
    outs = [("bitmap", 8 * ((n + 63) // 64), AL["d_bitmap"])]
    if with_status:
        outs.append(("status", n, AL["d_status"]))
    return Guarded(outs, fill, device=DEV)


def _check_verdicts(g, b, with_status, what):
    g.snapshot()
    bm = g.read("bitmap", np.uint64)
    assert np.array_equal(native.bitmap_to_bools(bm, b.n), b.verdict), (what, "verdict bits")
    assert tail_bits(bm, b.n) == 0, (what, "bits at and above n in the last word", hex(int(bm[-1])))
    if with_status:
        assert np.array_equal(g.read("status"), b.status), (what, "status")
    g.check_guards(str(what))
    return bm


# ---------------------------------------------------------------- cv_ed25519_verify_device
@pytest.mark.parametrize("form", list(FORMS))
def test_verify_device_outputs(engine, batches, form):
    """Prior contents, tail bits, guards, read-only inputs and alignment of cv_ed25519_verify_device: every size
    and both last-record kinds in one kernel form, over 0x00 and 0xFF, with and without d_status, on the context's
    stream and on a caller's."""
    own = torch.cuda.Stream(DEV)
    quad_max, tri_max = FORMS[form]
    with Options(engine, quad_max=quad_max, tri_max=tri_max):
        for (n, last), b in batches.items():
            for fill in FILLS:
                for with_status in (True, False):
                    for stream in (0, own.cuda_stream):
                        what = (form, n, last, hex(fill), "status" if with_status else "no status",
                                "own stream" if stream else "context stream")
                        g = _outputs(n, with_status, fill)
                        torch.cuda.synchronize()
                        engine.verify_device(0, n, b.p("pk"), b.p("sig"), b.p("arena"), b.p("off"), b.p("len"),
                                             g.ptr("bitmap"), g.ptr("status") if with_status else 0, stream)
                        torch.cuda.synchronize()
                        _check_verdicts(g, b, with_status, what)
                        b.assert_inputs_unchanged(what)


# ---------------------------------------------------------------- cv_ed25519_verify_device_timed
def _timed(engine, b, g, stream=0):
    ms = engine.verify_device_timed(0, b.n, b.p("pk"), b.p("sig"), b.p("arena"), b.p("off"), b.p("len"),
                                    g.ptr("bitmap"), stream)
    assert len(ms) == 3 and all(np.isfinite(x) and x >= 0.0 for x in ms), ms
    return ms


@pytest.mark.parametrize("form", list(FORMS))
def test_verify_device_timed_outputs(engine, batches, form):
    """The entry point behind the headline number against the corpus columns: as test_verify_device_outputs
    (no status), phase_ms finite and non-negative, and the bitmap equal to cv_ed25519_verify_device's."""
    quad_max, tri_max = FORMS[form]
    with Options(engine, quad_max=quad_max, tri_max=tri_max):
        for (n, last), b in batches.items():
            for fill in FILLS:
                what = (form, n, last, hex(fill), "timed")
                g = _outputs(n, False, fill)
                torch.cuda.synchronize()
                _timed(engine, b, g)
                torch.cuda.synchronize()
                bm = _check_verdicts(g, b, False, what)
                b.assert_inputs_unchanged(what)
            plain = _outputs(n, False, 0xFF)
            torch.cuda.synchronize()
            engine.verify_device(0, n, b.p("pk"), b.p("sig"), b.p("arena"), b.p("off"), b.p("len"), plain.ptr("bitmap"))
            torch.cuda.synchronize()
            assert np.array_equal(plain.read("bitmap", np.uint64), bm), (what, "timed and plain bitmaps differ")


@pytest.mark.parametrize("n", [4097, 32769])
def test_verify_device_timed_default_schedules(engine, corpus, arena_dev, n):
    """One record past each size at which the default options change schedule (tri up to 4,096, quad up to 32,768):
    the corpus tiled, the last record accepted, the buffer 0xFF."""
    b = _Batch(corpus, arena_dev, _rows(corpus, n, "accepted", seed=1))
    g = _outputs(n, False, 0xFF)
    torch.cuda.synchronize()
    _timed(engine, b, g)
    torch.cuda.synchronize()
    bm = _check_verdicts(g, b, False, ("timed", n))
    b.assert_inputs_unchanged(("timed", n))
    plain = _outputs(n, False, 0xFF)
    torch.cuda.synchronize()
    engine.verify_device(0, n, b.p("pk"), b.p("sig"), b.p("arena"), b.p("off"), b.p("len"), plain.ptr("bitmap"))
    torch.cuda.synchronize()
    assert np.array_equal(plain.read("bitmap", np.uint64), bm)
    plain.check_guards(f"plain {n}")


# ---------------------------------------------------------------- cv_ed25519_verify_device_keyed
@pytest.mark.parametrize("comb", ["quad_comb", "comb"])
def test_verify_device_keyed_outputs(engine, batches, comb):
    """cv_ed25519_verify_device_keyed with the keys of np.unique over the batch's pk rows (from two records up
    every batch holds a key that is not a point; a batch of one does when its record is the CV_SIG_BAD_KEY row):
    the quad comb (n <= CV_OPT_QUAD_MAX) and cv_comb_kernel (CV_OPT_QUAD_MAX = 0), phase_ms NULL and set."""
    with Options(engine, quad_max=(1 << 22) if comb == "quad_comb" else 0):
        for (n, last), b in batches.items():
            assert (b.status == native.CV_SIG_BAD_KEY).any() or (n == 1 and last == "accepted")
            for fill in FILLS:
                for timed in (False, True):
                    what = (comb, n, last, hex(fill), "phase_ms" if timed else "no phase_ms")
                    g = _outputs(n, True, fill)
                    torch.cuda.synchronize()
                    ms = engine.verify_device_keyed(0, n, b.nkeys, b.p("keys"), b.p("key_index"), b.p("sig"),
                                                    b.p("arena"), b.p("off"), b.p("len"), g.ptr("bitmap"),
                                                    g.ptr("status"), 0, timed=timed)
                    torch.cuda.synchronize()
                    if timed:
                        assert len(ms) == 4 and all(np.isfinite(x) and x >= 0.0 for x in ms), (what, ms)
                    _check_verdicts(g, b, True, what)
                    b.assert_inputs_unchanged(what, ("keys", "key_index", "sig", "arena", "off", "len"))


# ---------------------------------------------------------------- signing
SIGN_N = (1, 255, 256, 257)
SIGN_LENS = (0, 47, 48, 111, 112)        # SHA-512 block crossings of prefix || M (32 + len) and R || A || M (64 + len)
SIGNER_SEED = E.entropy_to_seed(20)


@pytest.fixture(scope="module")
def sign_case():
    """257 messages of the edge lengths at unaligned arena offsets (every residue mod 4), a seed per record, and
    the Python oracle's public keys and signatures: per-record seeds for cv_ed25519_sign_device, one seed for the
    signer.  A batch of n takes the first n records."""
    n = max(SIGN_N)
    rng = np.random.default_rng(8032)
    lens = np.array([SIGN_LENS[i % len(SIGN_LENS)] for i in range(n)], np.uint32)
    off = np.zeros(n, np.uint64)
    cur = 1
    for i in range(n):
        off[i] = cur
        cur += int(lens[i]) + 1 + i % 3
    assert {int(o) % 4 for o in off} == {0, 1, 2, 3}
    arena = rng.integers(0, 256, cur + 16, dtype=np.uint8)
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msgs = [arena[int(off[i]):int(off[i]) + int(lens[i])].tobytes() for i in range(n)]
    pk = np.frombuffer(b"".join(E.public_key_of(s.tobytes()) for s in seeds), np.uint8).reshape(n, 32)
    sig = np.frombuffer(b"".join(E.sign(s.tobytes(), m) for s, m in zip(seeds, msgs)), np.uint8).reshape(n, 64)
    ksig = np.frombuffer(b"".join(E.sign(SIGNER_SEED, m) for m in msgs), np.uint8).reshape(n, 64)
    t = {"seed": _up(seeds), "arena": _up(arena), "off": _up(off), "len": _up(lens)}
    return dict(pk=pk, sig=sig, ksig=ksig, t=t, orig={k: v.clone() for k, v in t.items()})


def _sign_inputs_unchanged(c, what):
    for k, v in c["t"].items():
        assert torch.equal(v, c["orig"][k]), (what, f"input {k} was written")


def test_sign_device_outputs(engine, sign_case):
    """cv_ed25519_sign_device: d_pk and d_sig at 16 mod 32 over 0xFF and 0x00 hold the oracle's bytes; guards and
    inputs intact."""
    c = sign_case
    t = c["t"]
    for n in SIGN_N:
        for fill in (0xFF, 0x00):
            what = ("sign_device", n, hex(fill))
            g = Guarded([("pk", 32 * n, AL["d_pk"]), ("sig", 64 * n, AL["d_sig"])], fill, device=DEV)
            torch.cuda.synchronize()
            engine.sign_device(0, n, t["seed"].data_ptr(), t["arena"].data_ptr(), t["off"].data_ptr(),
                               t["len"].data_ptr(), g.ptr("pk"), g.ptr("sig"))
            torch.cuda.synchronize()
            g.snapshot()
            assert np.array_equal(g.read("pk", shape=(n, 32)), c["pk"][:n]), what
            assert np.array_equal(g.read("sig", shape=(n, 64)), c["sig"][:n]), what
            g.check_guards(str(what))
            _sign_inputs_unchanged(c, what)


def test_sign_keyed_device_outputs(engine, sign_case):
    """cv_ed25519_sign_keyed_device: d_sig at 16 mod 32 over 0xFF and 0x00 holds the oracle's signatures under the
    signer's seed; guards and inputs intact."""
    c = sign_case
    t = c["t"]
    with native.Signer(engine, SIGNER_SEED) as s:
        assert s.public_key == E.public_key_of(SIGNER_SEED)
        for n in SIGN_N:
            for fill in (0xFF, 0x00):
                what = ("sign_keyed_device", n, hex(fill))
                g = Guarded([("sig", 64 * n, AL["d_sig"])], fill, device=DEV)
                torch.cuda.synchronize()
                s.sign_device(0, n, t["arena"].data_ptr(), t["off"].data_ptr(), t["len"].data_ptr(), g.ptr("sig"))
                torch.cuda.synchronize()
                g.snapshot()
                assert np.array_equal(g.read("sig", shape=(n, 64)), c["ksig"][:n]), what
                g.check_guards(str(what))
                _sign_inputs_unchanged(c, what)


# ---------------------------------------------------------------- cv_merkle_tx_ids_device
LEAF_SPAN = 2 * 256                      # leaves per workgroup of the leaf kernel: 2 x CV_LEAF_BLOCK


def _merkle_case(nleaves):
    """Transactions of 0, 1, 2, 3, 64 and 65 leaves, then ragged ones (empty ones among them) up to exactly nleaves,
    and an empty one last; leaf lengths 0, 55, 56, 64 (the SHA-256 padding edges) among others and one leaf of 65
    blocks (past the leaf kernel's 63-block bucket), at unaligned offsets with gaps."""
    rng = np.random.default_rng(nleaves)
    counts = [0, 1, 2, 3, 64, 65]
    while sum(counts) < nleaves:
        counts.append(min(int(rng.integers(0, 9)), nleaves - sum(counts)))
    counts.append(0)
    begin = np.zeros(len(counts) + 1, np.uint32)
    begin[1:] = np.cumsum(counts)
    assert int(begin[-1]) == nleaves
    edge = (0, 55, 56, 64, 1, 63, 119, 120, 300)
    lens = np.array([edge[i % len(edge)] for i in range(nleaves)], np.uint32)
    lens[7] = 4100
    assert (int(lens[7]) + 9 + 63) // 64 >= 63
    off = np.zeros(nleaves, np.uint64)
    cur = 3
    for i in range(nleaves):
        off[i] = cur
        cur += int(lens[i]) + i % 4
    arena = rng.integers(0, 256, cur + 16, dtype=np.uint8)
    return arena, off, lens, begin


@pytest.mark.parametrize("nleaves", [LEAF_SPAN - 1, LEAF_SPAN, LEAF_SPAN + 1])
def test_merkle_device_outputs(engine, oracle_c, nleaves):
    """cv_merkle_tx_ids_device one leaf below, at and above the leaf kernel's span: ids and status equal the C
    oracle's over 0x00 and 0xFF, d_tx_status NULL and set; an empty transaction's id is 32 zero bytes whatever the
    buffer held; nothing is written around d_ids, d_tx_status or the nleaves * 32 bytes of d_workspace; the inputs
    are unchanged."""
    arena, off, lens, begin = _merkle_case(nleaves)
    ntx = len(begin) - 1
    ref_ids, ref_st = oracle_c.merkle_tx_ids(arena, off, lens, begin)
    empty = np.diff(begin.astype(np.int64)) == 0
    assert empty.sum() >= 2 and np.array_equal(ref_st, empty.astype(np.uint8))
    t = {"arena": _up(arena), "off": _up(off), "len": _up(lens), "begin": _up(begin)}
    orig = {k: v.clone() for k, v in t.items()}
    for fill in FILLS:
        for with_status in (True, False):
            what = ("merkle_device", nleaves, hex(fill), "status" if with_status else "no status")
            outs = [("ids", 32 * ntx, AL["d_ids"]), ("workspace", 32 * nleaves, AL["d_workspace"])]
            if with_status:
                outs.append(("status", ntx, AL["d_tx_status"]))
            g = Guarded(outs, fill, device=DEV)
            torch.cuda.synchronize()
            engine.merkle_device(0, ntx, nleaves, t["arena"].data_ptr(), t["off"].data_ptr(), t["len"].data_ptr(),
                                 t["begin"].data_ptr(), g.ptr("workspace"), g.ptr("ids"),
                                 g.ptr("status") if with_status else 0)
            torch.cuda.synchronize()
            g.snapshot()
            ids = g.read("ids", shape=(ntx, 32))
            assert np.array_equal(ids, ref_ids), what
            assert not ids[empty].any(), (what, "the id of an empty transaction is not zero")
            if with_status:
                assert np.array_equal(g.read("status"), ref_st), what
            g.check_guards(str(what))
            for k, v in t.items():
                assert torch.equal(v, orig[k]), (what, f"input {k} was written")


# ---------------------------------------------------------------- calls that touch nothing
def test_device_calls_of_nothing_touch_nothing(engine, batches):
    """n == 0 (ntx == 0) on every device entry point returns CV_OK and leaves every output byte as it was."""
    lib, h = engine._lib, engine._h
    b = batches[(5, "accepted")]
    g = Guarded([("bitmap", 8, 8), ("status", 5, 1), ("pk", 32, 16), ("sig", 64, 16), ("ids", 32, 16),
                 ("workspace", 32, 16)], 0xA5, device=DEV)
    torch.cuda.synchronize()
    ms = (ctypes.c_float * 4)(-1.0, -1.0, -1.0, -1.0)
    assert lib.cv_ed25519_verify_device(h, 0, 0, b.p("pk"), b.p("sig"), b.p("arena"), b.p("off"), b.p("len"),
                                        g.ptr("bitmap"), g.ptr("status"), None) == 0
    assert lib.cv_ed25519_verify_device_timed(h, 0, 0, b.p("pk"), b.p("sig"), b.p("arena"), b.p("off"), b.p("len"),
                                              g.ptr("bitmap"), None, ctypes.cast(ms, ctypes.POINTER(ctypes.c_float))) == 0
    assert list(ms)[:3] == [0.0, 0.0, 0.0]
    assert lib.cv_ed25519_verify_device_keyed(h, 0, 0, b.nkeys, b.p("keys"), b.p("key_index"), b.p("sig"),
                                              b.p("arena"), b.p("off"), b.p("len"), g.ptr("bitmap"), g.ptr("status"),
                                              None, None) == 0
    assert lib.cv_ed25519_sign_device(h, 0, 0, b.p("pk"), b.p("arena"), b.p("off"), b.p("len"), g.ptr("pk"),
                                      g.ptr("sig"), None) == 0
    with native.Signer(engine, SIGNER_SEED) as s:
        assert lib.cv_ed25519_sign_keyed_device(h, 0, s._h, 0, b.p("arena"), b.p("off"), b.p("len"), g.ptr("sig"),
                                                None) == 0
    assert lib.cv_merkle_tx_ids_device(h, 0, 0, 0, b.p("arena"), b.p("off"), b.p("len"), b.p("len"),
                                       g.ptr("workspace"), g.ptr("ids"), g.ptr("status"), None) == 0
    torch.cuda.synchronize()
    g.snapshot()
    for name in g.order:
        assert g.untouched(name), name
    g.check_guards("n == 0")
