"""The output contract of the host-buffer C-ABI (include/cordaverify.h), through raw ctypes (native.load()) — not
the binding's wrappers, which hand the library zeroed arrays of exactly the right size.

Every output is carved from a guarded numpy buffer (tests/guarded.py) filled with 0xA5 and again with 0x5A, at the
natural alignment of its C type and no more (uint64 at 8 mod 16, uint32 at 4 mod 8, bytes at an odd address):
outputs may hold anything on entry, tail bits of the bitmap are written as zero, the records the header promises as
zero are zero, nothing around an output is written, and the calls the header says touch nothing leave every byte.
One small batch per entry point: the kernels' own edges are tests/test_gpu_output_contract.py's; this file is about
the copy-out and assembly code of each host path.
"""
import ctypes

import numpy as np
import pytest

import ed25519_ref as E
import pmt_build_cases as PC
import uniq_cases as UC
from corda_amd import native
from corda_amd.uniqueness import InMemoryUniquenessProvider
from guarded import Guarded, Options, corpus_rows, tail_bits

pytestmark = pytest.mark.gpu

FILLS = (0xA5, 0x5A)
CV_E_ARGS, CV_E_OOM = -3, -4
SIGNER_SEED = E.entropy_to_seed(20)


def _p(a):
    return None if a is None else a.ctypes.data


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


# ---------------------------------------------------------------- verify
class _VBatch:
    def __init__(self, engine, corpus, n):
        rows = corpus_rows(corpus, n, "accepted", seed=2)
        self.n = n
        self.verdict = corpus["verdict"][rows].astype(bool)
        self.status = corpus["status"][rows].astype(np.uint8)
        assert self.verdict[-1] and (self.status == native.CV_SIG_BAD_KEY).any()
        pk = _c(corpus["pk"][rows], np.uint8)
        keys, inv = np.unique(pk, axis=0, return_inverse=True)
        host = {"pk": pk, "sig": _c(corpus["sig"][rows], np.uint8), "arena": _c(corpus["arena"], np.uint8),
                "off": _c(corpus["off"][rows], np.uint64), "len": _c(corpus["len"][rows], np.uint32),
                "keys": _c(keys, np.uint8), "key_index": _c(inv.reshape(-1), np.uint32)}
        self.nkeys = len(keys)
        self.inputs = {False: host, True: {k: engine.host_copy(v) for k, v in host.items()}}
        self.orig = {k: v.copy() for k, v in host.items()}

    def assert_inputs_unchanged(self, what):
        for pinned, arrays in self.inputs.items():
            for k, v in arrays.items():
                assert np.array_equal(v, self.orig[k]), (what, f"input {k} was written")


@pytest.fixture(scope="module")
def vbatches(engine, corpus):
    return {n: _VBatch(engine, corpus, n) for n in (5, 65, 4097)}


def _verify_call(lib, h, ep, b, a, bm, st):
    n, arena_bytes = b.n, a["arena"].size
    if ep == "batch":
        return lib.cv_ed25519_verify_batch(h, n, _p(a["pk"]), _p(a["sig"]), _p(a["arena"]), _p(a["off"]), _p(a["len"]),
                                           bm, st)
    if ep == "ex":
        return lib.cv_ed25519_verify_batch_ex(h, n, _p(a["pk"]), _p(a["sig"]), _p(a["arena"]), arena_bytes, _p(a["off"]),
                                              _p(a["len"]), bm, st, None)
    if ep == "async":
        t = ctypes.c_uint64(0)
        rc = lib.cv_ed25519_verify_batch_async(h, n, _p(a["pk"]), _p(a["sig"]), _p(a["arena"]), _p(a["off"]),
                                               _p(a["len"]), bm, st, ctypes.byref(t))
        return rc if rc != 0 else lib.cv_wait(h, t)
    assert ep == "keyed"
    return lib.cv_ed25519_verify_batch_keyed(h, n, b.nkeys, _p(a["keys"]), _p(a["key_index"]), _p(a["sig"]),
                                             _p(a["arena"]), _p(a["off"]), _p(a["len"]), bm, st)


def _verify_outputs(engine, n, with_status, fill, pinned):
    outs = [("bitmap", 8 * ((n + 63) // 64), 8)]
    if with_status:
        outs.append(("status", n, 1))
    return Guarded(outs, fill, alloc=(lambda nb: engine.host_empty(nb)) if pinned else None)


@pytest.mark.parametrize("ep", ["batch", "ex", "async", "keyed"])
def test_verify_host_outputs(engine, vbatches, ep):
    """cv_ed25519_verify_batch, _ex, _async + cv_wait and _keyed at 5, 65 and 4,097 records: each small-path form
    (CV_OPT_SMALL_ZERO_COPY 0, 1, 2), pinned and pageable arrays, status NULL and set — exact verdicts and status,
    zero tail bits, intact guards and inputs.  At 4,097 the plain entry points run with the automatic keyed path on
    and off (the corpus's keys repeat)."""
    lib, h = engine._lib, engine._h
    for n, b in vbatches.items():
        for szc in (0, 1, 2):
            for auto_keyed in ((1, 0) if n > 4096 and ep != "keyed" else (1,)):
                with Options(engine, small_zero_copy=szc, auto_keyed=auto_keyed):
                    for pinned in (False, True):
                        for with_status in (True, False):
                            for fill in FILLS:
                                what = (ep, n, f"zero_copy={szc}", f"auto_keyed={auto_keyed}",
                                        "pinned" if pinned else "pageable", "status" if with_status else "no status",
                                        hex(fill))
                                g = _verify_outputs(engine, n, with_status, fill, pinned)
                                rc = _verify_call(lib, h, ep, b, b.inputs[pinned], g.ptr("bitmap"),
                                                  g.ptr("status") if with_status else None)
                                assert rc == 0, (what, rc)
                                bm = g.read("bitmap", np.uint64)
                                assert np.array_equal(native.bitmap_to_bools(bm, n), b.verdict), what
                                assert tail_bits(bm, n) == 0, (what, hex(int(bm[-1])))
                                if with_status:
                                    assert np.array_equal(g.read("status"), b.status), what
                                g.check_guards(str(what))
        b.assert_inputs_unchanged((ep, n))


# ---------------------------------------------------------------- Merkle ids and whole transactions
def _tx_case(engine, oracle_c, corpus):
    """40 ragged transactions (0..12 leaves, empty ones among them; 0..5 signatures, none for some) signed over the
    C oracle's ids, then one S corrupted in every seventh signature and every eleventh key replaced by a corpus
    key that is not a point.  The reference: the C oracle's ids, statuses and verdicts."""
    rng = np.random.default_rng(404)
    ntx = 40
    counts = rng.integers(0, 13, ntx)
    counts[:5] = [0, 1, 2, 3, 0]
    begin = np.zeros(ntx + 1, np.uint32)
    begin[1:] = np.cumsum(counts)
    nl = int(begin[-1])
    lens = rng.integers(0, 300, nl).astype(np.uint32)
    lens[-1] = 17
    off = np.zeros(nl, np.uint64)
    off[1:] = np.cumsum(lens[:-1] + 1)
    arena = rng.integers(0, 256, int(off[-1]) + int(lens[-1]), dtype=np.uint8)     # ends with the last leaf's last byte
    ids, st = oracle_c.merkle_tx_ids(arena, off, lens, begin)
    scount = rng.integers(0, 6, ntx)
    scount[:5] = [2, 0, 1, 3, 0]
    tsb = np.zeros(ntx + 1, np.uint32)
    tsb[1:] = np.cumsum(scount)
    nsig = int(tsb[-1])
    tx_of = np.repeat(np.arange(ntx), scount)
    msg_arena = np.concatenate([ids.reshape(-1), np.zeros(16, np.uint8)])
    msg_off, msg_len = tx_of.astype(np.uint64) * 32, np.full(nsig, 32, np.uint32)
    pk, sig = engine.sign_batch(rng.integers(0, 256, (nsig, 32), dtype=np.uint8), msg_arena, msg_off, msg_len)
    sig[::7, 40] ^= 0x10
    bad = np.nonzero(corpus["status"] == 1)[0]
    kbad = np.arange(3, nsig, 11)
    pk[kbad] = corpus["pk"][bad[kbad % len(bad)]]
    verdict, sstat = oracle_c.verify_batch(pk, sig, msg_arena, msg_off, msg_len)
    ok = (st == 0) & (scount > 0)
    all_valid = np.ones(ntx, bool)
    np.logical_and.at(all_valid, tx_of, verdict.astype(bool))
    ok &= all_valid
    assert 0 < ok.sum() < ntx and sstat.sum() > 0 and st.sum() >= 2
    return dict(ntx=ntx, nsig=nsig, arena=arena, off=off, len=lens, begin=begin, pk=pk, sig=sig, tsb=tsb,
                ids=ids, st=st, sst=sstat, ok=ok.astype(np.uint8))


@pytest.fixture(scope="module")
def tx_case(engine, oracle_c, corpus):
    return _tx_case(engine, oracle_c, corpus)


@pytest.mark.parametrize("ep", ["ex", "bounded"])
def test_merkle_host_outputs(engine, tx_case, ep):
    """cv_merkle_tx_ids_ex / _bounded: ids and tx_status over the poison equal the C oracle's, an empty
    transaction's id is 32 zero bytes, and with the optional tx_status NULL the ids are the same bytes."""
    lib, h, c = engine._lib, engine._h, tx_case
    ntx = c["ntx"]
    for fill in FILLS:
        seen = []
        for with_status in (True, False):
            what = ("merkle", ep, hex(fill), with_status)
            outs = [("ids", 32 * ntx, 1)] + ([("tx_status", ntx, 1)] if with_status else [])
            g = Guarded(outs, fill)
            st = g.ptr("tx_status") if with_status else None
            if ep == "ex":
                rc = lib.cv_merkle_tx_ids_ex(h, ntx, _p(c["arena"]), _p(c["off"]), _p(c["len"]), _p(c["begin"]),
                                             g.ptr("ids"), st)
            else:
                rc = lib.cv_merkle_tx_ids_bounded(h, ntx, _p(c["arena"]), c["arena"].size, _p(c["off"]), _p(c["len"]),
                                                  _p(c["begin"]), g.ptr("ids"), st, None)
            assert rc == 0, what
            ids = g.read("ids", shape=(ntx, 32))
            assert np.array_equal(ids, c["ids"]), what
            assert not ids[c["st"] == 1].any(), (what, "the id of an empty transaction is not zero")
            if with_status:
                assert np.array_equal(g.read("tx_status"), c["st"]), what
            g.check_guards(str(what))
            seen.append(ids)
        assert np.array_equal(seen[0], seen[1])


@pytest.mark.parametrize("ep", ["plain", "ex"])
def test_verify_transactions_host_outputs(engine, tx_case, ep):
    """cv_verify_transactions / _ex: all outputs over the poison equal the oracle's; then ids, tx_status and
    sig_status NULL in turn — the remaining outputs are the bytes of the all-outputs call."""
    lib, h, c = engine._lib, engine._h, tx_case
    ntx, nsig = c["ntx"], c["nsig"]
    sizes = {"ids": 32 * ntx, "tx_status": ntx, "sig_status": nsig, "tx_ok": ntx}

    def call(g, absent):
        ptr = {k: (None if k == absent else g.ptr(k)) for k in sizes}
        args = [_p(c["off"]), _p(c["len"]), _p(c["begin"]), _p(c["pk"]), _p(c["sig"]), _p(c["tsb"]), ptr["ids"],
                ptr["tx_status"], ptr["sig_status"], ptr["tx_ok"]]
        if ep == "plain":
            return lib.cv_verify_transactions(h, ntx, _p(c["arena"]), *args)
        return lib.cv_verify_transactions_ex(h, ntx, _p(c["arena"]), c["arena"].size, *args, None)

    for fill in FILLS:
        full = None
        for absent in (None, "ids", "tx_status", "sig_status"):
            what = ("verify_transactions", ep, hex(fill), f"NULL: {absent}")
            g = Guarded([(k, nb, 1) for k, nb in sizes.items() if k != absent], fill)
            assert call(g, absent) == 0, what
            got = {k: g.read(k) for k in sizes if k != absent}
            g.check_guards(str(what))
            if absent is None:
                full = got
                assert np.array_equal(got["ids"].reshape(ntx, 32), c["ids"]), what
                assert np.array_equal(got["tx_status"], c["st"]), what
                assert np.array_equal(got["sig_status"], c["sst"]), what
                assert np.array_equal(got["tx_ok"], c["ok"]), what
            else:
                for k, v in got.items():
                    assert np.array_equal(v, full[k]), (what, k)


# ---------------------------------------------------------------- partial Merkle trees
def test_partial_merkle_verify_host_outputs(engine):
    """cv_partial_merkle_verify over the golden fixture (447 trees, the malformed encodings among them; child indices
    are absolute, so the fixture goes in whole): verdict and status (NULL and set) over the poison equal the
    fixture's columns."""
    import os
    c = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "partial_merkle_cases.npz")))
    lib, h = engine._lib, engine._h
    kind, left, right = _c(c["kind"], np.uint8), _c(c["left"], np.uint32), _c(c["right"], np.uint32)
    hashes, tb, root = _c(c["leaf_hash"], np.uint8), _c(c["tree_begin"], np.uint32), _c(c["root"], np.uint8)
    check, cb = _c(c["check"], np.uint8), _c(c["check_begin"], np.uint32)
    want_v, want_s = c["verdict"], c["status"]
    m = len(want_v)
    assert (want_s == 2).sum() >= 3 and want_v.sum() >= 3 and (want_v == 0).sum() > (want_s == 2).sum()
    for fill in FILLS:
        for with_status in (True, False):
            what = ("partial_merkle_verify", hex(fill), with_status)
            g = Guarded([("verdict", m, 1)] + ([("status", m, 1)] if with_status else []), fill)
            rc = lib.cv_partial_merkle_verify(h, m, len(kind), _p(kind), _p(left), _p(right), _p(hashes), _p(tb),
                                              _p(root), len(check), _p(check), _p(cb), g.ptr("verdict"),
                                              g.ptr("status") if with_status else None)
            assert rc == 0, what
            assert np.array_equal(g.read("verdict"), want_v), what
            if with_status:
                assert np.array_equal(g.read("status"), want_s), what
            g.check_guards(str(what))


def _build_batches():
    """Two batches of the SAME layout (40 transactions of 8 leaves, the same number of include hashes): the second
    takes the include masks in reverse order, so a node that is a Leaf with a hash in one is a Node in the other and
    what the first call left in the engine's workspace differs from what the second must write.  A third includes
    every leaf: it needs exactly cv_partial_merkle_build_bound nodes."""
    leaves = [[PC.M.sha256(bytes([99, t, i])) for i in range(8)] for t in range(40)]
    masks = [(37 * t + 1) % 256 for t in range(40)]

    def batch(ms):
        return PC.batch_of([(lv, [lv[i] for i in range(8) if (m >> i) & 1], [(m >> i) & 1 for i in range(8)])
                            for lv, m in zip(leaves, ms)])
    return batch(masks), batch(masks[::-1]), batch([255] * 40)


NODE_OUT = ("kind", "left", "right", "node_hash")


def _build_call(lib, h, which, b, blobs, cap, g, want_ids=True):
    nn = ctypes.c_size_t(0xDEAD)
    outs = [g.ptr("kind"), g.ptr("left"), g.ptr("right"), g.ptr("node_hash"), g.ptr("tree_begin"),
            g.ptr("ids") if want_ids else None, g.ptr("status"), ctypes.byref(nn)]
    if which == "partial_merkle_build":
        rc = lib.cv_partial_merkle_build(h, b["ntx"], _p(b["leaf_hash"]), _p(b["txb"]), _p(b["include"]),
                                         _p(b["inc_begin"]), cap, *outs)
    else:
        arena, off, ln = blobs
        rc = lib.cv_filtered_build(h, b["ntx"], _p(arena), arena.size, _p(off), _p(ln), _p(b["txb"]), _p(b["keep"]),
                                   cap, *outs)
    return rc, nn.value


def _filtered_twin(leaf_blobs, masks):
    """The batch over blobs: leaves are SHA-256 of the blobs, includes the kept leaves' hashes."""
    cases = []
    for blobs, m in zip(leaf_blobs, masks):
        lv = [PC.M.sha256(x) for x in blobs]
        keep = [(m >> i) & 1 for i in range(len(lv))]
        cases.append((lv, [x for x, k in zip(lv, keep) if k], keep))
    return PC.batch_of(cases)


@pytest.mark.parametrize("which", ["partial_merkle_build", "cv_filtered_build"])
def test_build_host_outputs(engine, which):
    """cv_partial_merkle_build and cv_filtered_build with nodes_cap exactly the bound and one node short.  Exactly the
    bound: every array equals the oracle's over the poison — node_hash of a Node is 32 zero bytes and left / right of
    a leaf are 0 — on two batches of one layout that put Nodes where the other has Leaves, and on a batch that
    includes every leaf and so fills the bound; entries past *nnodes are not written.  One short (of the bound for
    the batch that fills it, of the nodes the batch needs for the others): CV_E_ARGS, the node arrays untouched,
    tree_begin, status, ids and *nnodes written."""
    lib, h = engine._lib, engine._h
    rng = np.random.default_rng(77)
    masks = [(37 * t + 1) % 256 for t in range(40)]
    if which == "partial_merkle_build":
        pair = _build_batches()
        blobs = None
    else:
        leaf_blobs = [[rng.bytes(int(rng.integers(1, 200))) for _ in range(8)] for _ in range(40)]
        flat = [x for tx in leaf_blobs for x in tx]
        ln = np.array([len(x) for x in flat], np.uint32)
        off = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.uint64)
        blobs = (np.frombuffer(b"".join(flat), np.uint8).copy(), off, ln)
        pair = (_filtered_twin(leaf_blobs, masks), _filtered_twin(leaf_blobs, masks[::-1]),
                _filtered_twin(leaf_blobs, [255] * 40))
    for b in pair:
        ntx = b["ntx"]
        bound = native.partial_merkle_build_bound(b["txb"])
        nn_want = int(b["tree_begin"][-1])
        assert 0 < nn_want <= bound and (b["kind"] == 2).sum() > 40 and (b["status"] == 0).all()
        assert (nn_want == bound) == (b is pair[2])          # the last batch includes every leaf: exactly the bound

        def outputs(cap, fill):
            return Guarded([("kind", cap, 1), ("left", 4 * cap, 4), ("right", 4 * cap, 4), ("node_hash", 32 * cap, 1),
                            ("tree_begin", 4 * (ntx + 1), 4), ("ids", 32 * ntx, 1), ("status", ntx, 1)], fill)

        for fill in FILLS:
            what = (which, hex(fill), "cap = bound")
            g = outputs(bound, fill)
            rc, nn = _build_call(lib, h, which, b, blobs, bound, g)
            assert rc == 0 and nn == nn_want, (what, rc, nn)
            kind = g.read("kind")
            left, right = g.read("left", np.uint32), g.read("right", np.uint32)
            hashes = g.read("node_hash", shape=(bound, 32))
            assert np.array_equal(kind[:nn], b["kind"]), what
            assert np.array_equal(left[:nn], b["left"]) and np.array_equal(right[:nn], b["right"]), what
            assert np.array_equal(hashes[:nn], b["node_hash"]), what
            assert not hashes[:nn][kind[:nn] == 2].any(), (what, "node_hash of a Node is not zero")
            assert not left[:nn][kind[:nn] != 2].any() and not right[:nn][kind[:nn] != 2].any(), what
            fill_word = np.frombuffer(bytes([fill] * 4), np.uint32)[0]
            assert (kind[nn:] == fill).all() and (left[nn:] == fill_word).all() and (right[nn:] == fill_word).all() \
                and (hashes[nn:] == fill).all(), (what, "entries past *nnodes were written")
            assert np.array_equal(g.read("tree_begin", np.uint32), b["tree_begin"]), what
            assert np.array_equal(g.read("ids", shape=(ntx, 32)), b["ids"]), what
            assert np.array_equal(g.read("status"), b["status"]), what
            g.check_guards(str(what))

            what = (which, hex(fill), "cap one short")
            g = outputs(nn_want - 1, fill)
            rc, nn = _build_call(lib, h, which, b, blobs, nn_want - 1, g)
            assert rc == CV_E_ARGS and nn == nn_want, (what, rc, nn)
            for name in NODE_OUT:
                assert g.untouched(name), (what, name)
            assert np.array_equal(g.read("tree_begin", np.uint32), b["tree_begin"]), what
            assert np.array_equal(g.read("ids", shape=(ntx, 32)), b["ids"]), what
            assert np.array_equal(g.read("status"), b["status"]), what
            g.check_guards(str(what))


# ---------------------------------------------------------------- signing
def _sign_case():
    n = 70
    rng = np.random.default_rng(70)
    lens = rng.integers(0, 130, n).astype(np.uint32)
    lens[:5] = [0, 47, 48, 111, 112]
    lens[-1] = 33
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(lens[:-1] + 1)
    arena = rng.integers(0, 256, int(off[-1]) + int(lens[-1]), dtype=np.uint8)    # ends with the last message
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msgs = [arena[int(o):int(o) + int(k)].tobytes() for o, k in zip(off, lens)]
    return n, seeds, arena, off, lens, msgs


def test_sign_host_outputs(engine):
    """cv_ed25519_sign_batch and cv_ed25519_sign_keyed: 70 messages, outputs over the
    poison equal oracle/ed25519_ref.py's; guards intact.  cv_ed25519_sign_keyed past its arena bound (one byte
    short): CV_E_ARGS and no output byte written."""
    lib, h = engine._lib, engine._h
    n, seeds, arena, off, lens, msgs = _sign_case()
    want_pk = np.frombuffer(b"".join(E.public_key_of(s.tobytes()) for s in seeds), np.uint8).reshape(n, 32)
    want_sig = np.frombuffer(b"".join(E.sign(s.tobytes(), m) for s, m in zip(seeds, msgs)), np.uint8).reshape(n, 64)
    want_ksig = np.frombuffer(b"".join(E.sign(SIGNER_SEED, m) for m in msgs), np.uint8).reshape(n, 64)
    with native.Signer(engine, SIGNER_SEED) as s:
        for fill in FILLS:
            g = Guarded([("pk", 32 * n, 1), ("sig", 64 * n, 1)], fill)
            assert lib.cv_ed25519_sign_batch(h, n, _p(seeds), _p(arena), _p(off), _p(lens), g.ptr("pk"), g.ptr("sig")) == 0
            assert np.array_equal(g.read("pk", shape=(n, 32)), want_pk)
            assert np.array_equal(g.read("sig", shape=(n, 64)), want_sig)
            g.check_guards(f"sign_batch {fill:#x}")
            g = Guarded([("sig", 64 * n, 1)], fill)
            assert lib.cv_ed25519_sign_keyed(h, s._h, n, _p(arena), arena.size, _p(off), _p(lens), g.ptr("sig")) == 0
            assert np.array_equal(g.read("sig", shape=(n, 64)), want_ksig)
            g.check_guards(f"sign_keyed {fill:#x}")
            g.refill()
            assert lib.cv_ed25519_sign_keyed(h, s._h, n, _p(arena), arena.size - 1, _p(off), _p(lens),
                                             g.ptr("sig")) == CV_E_ARGS
            assert g.untouched("sig")
            g.check_guards(f"sign_keyed past the bound {fill:#x}")


# ---------------------------------------------------------------- the uniqueness set
UNIQ_OUT = ("tx_status", "state_conflict", "cons_id", "cons_index", "cons_caller")


def _uniq_outputs(ntx, ns, fill):
    return Guarded([("tx_status", ntx, 1), ("state_conflict", ns, 1), ("cons_id", 32 * ns, 1), ("cons_index", 4 * ns, 4),
                    ("cons_caller", 4 * ns, 4)], fill)


def _uniq_commit(lib, s, f, g):
    return lib.cv_uniq_commit_batch(s._h, f["ntx"], _p(f["key"]), _p(f["begin"]), _p(f["id"]), _p(f["caller"]),
                                    _p(f["enable"]), g.ptr("tx_status"), g.ptr("state_conflict"), g.ptr("cons_id"),
                                    g.ptr("cons_index"), g.ptr("cons_caller"))


def _uniq_read(g, ns):
    return dict(tx_status=g.read("tx_status"), state_conflict=g.read("state_conflict"),
                cons_id=g.read("cons_id", shape=(ns, 32)), cons_index=g.read("cons_index", np.uint32),
                cons_caller=g.read("cons_caller", np.uint32))


def _uniq_lookup(lib, s, keys, fill, what):
    n = len(keys)
    g = Guarded([("found", n, 1), ("cons_id", 32 * n, 1), ("cons_index", 4 * n, 4), ("cons_caller", 4 * n, 4)], fill)
    assert lib.cv_uniq_lookup(s._h, n, _p(keys), g.ptr("found"), g.ptr("cons_id"), g.ptr("cons_index"),
                              g.ptr("cons_caller")) == 0, what
    g.check_guards(str(what))
    return g.read("found"), g.read("cons_id", shape=(n, 32)), g.read("cons_index", np.uint32), g.read("cons_caller", np.uint32)


@pytest.mark.parametrize("fill", FILLS, ids=hex)
def test_uniq_host_outputs(engine, fill):
    """cv_uniq_commit_batch and cv_uniq_lookup against the InMemoryUniquenessProvider mirror (tests/uniq_cases.py),
    outputs over the poison.  Three commits of ONE shape into one set — 60 requests x 2 states accepted, the same
    states again (every record a conflict's), then fresh states (every record zero again, where the call before
    left conflicts in the set's workspace) — and a mixed batch with accepted, conflicting and skipped requests;
    lookups of present keys, then as many absent ones, then mixed.  A CV_E_OOM commit writes no output byte."""
    lib = engine._lib
    K = UC.key_of
    first = [([K("oc", 2 * t), K("oc", 2 * t + 1)], UC.tx_id_of("oc", t), t % 5 + 1, True) for t in range(60)]
    again = [(ks, UC.tx_id_of("oc", 100 + t), t % 3 + 7, True) for t, (ks, _, _, _) in enumerate(first)]
    fresh = [([K("oc", 1000 + 2 * t), K("oc", 1001 + 2 * t)], UC.tx_id_of("oc", 200 + t), t % 4 + 1, True)
             for t in range(60)]
    mixed = [([K("oc", 3 * t if t % 2 == 0 else 7000 + t), K("oc", 5000 + t), K("oc", 5000 + t // 2)],
              UC.tx_id_of("oc", 300 + t), t + 1, t % 4 != 3)
             for t in range(30)]
    oracle = InMemoryUniquenessProvider()
    with native.UniquenessSet(engine, 1024) as s:
        for name, batch in (("first", first), ("again", again), ("fresh", fresh), ("mixed", mixed)):
            f = UC.flatten(batch)
            want = UC.expect(oracle, batch)
            g = _uniq_outputs(f["ntx"], f["nstates"], fill)
            assert _uniq_commit(lib, s, f, g) == 0, name
            got = _uniq_read(g, f["nstates"])
            UC.assert_same(got, want, name)
            zero = got["state_conflict"] == 0
            assert not got["cons_id"][zero].any() and not got["cons_index"][zero].any() \
                and not got["cons_caller"][zero].any(), (name, "a state without a conflict has a non-zero record")
            g.check_guards(f"commit {name}")
            if name == "again":
                assert (got["tx_status"] == UC.CONFLICT).all() and got["state_conflict"].all() and got["cons_caller"].all()
            if name == "fresh":
                assert (got["tx_status"] == UC.OK).all()
            if name == "mixed":
                assert {int(x) for x in got["tx_status"]} == {UC.OK, UC.CONFLICT, UC.SKIPPED}
        present = UC.keys_array([k for ks, _, _, _ in first for k in ks])
        absent = UC.keys_array([K("absent", i) for i in range(len(present))])
        both = np.concatenate([present[::2], absent[::2]])[np.random.default_rng(1).permutation(len(present))]
        for name, keys in (("present", present), ("absent", absent), ("both", both)):
            got = _uniq_lookup(lib, s, keys, fill, ("lookup", name))
            want = UC.expect_lookup(oracle, [k.tobytes() for k in keys])
            for a, b, col in zip(got, want, ("found", "id", "index", "caller")):
                assert np.array_equal(a, b), (name, col)
            miss = got[0] == 0
            assert not got[1][miss].any() and not got[2][miss].any() and not got[3][miss].any(), name
        assert _uniq_lookup(lib, s, present, fill, "present")[0].all() and not _uniq_lookup(lib, s, absent, fill, "absent")[0].any()
    # past the capacity: CV_E_OOM before any output is written
    with native.UniquenessSet(engine, 16) as s:
        f = UC.flatten(first)
        g = _uniq_outputs(f["ntx"], f["nstates"], fill)
        assert _uniq_commit(lib, s, f, g) == CV_E_OOM
        for name in UNIQ_OUT:
            assert g.untouched(name), name
        g.check_guards("commit past the capacity")


# ---------------------------------------------------------------- calls that touch nothing
def test_host_calls_of_nothing_touch_nothing(engine, vbatches, tx_case):
    """n == 0 (ntx, ntrees == 0) on every host entry point returns CV_OK and leaves every output byte as it was."""
    lib, h = engine._lib, engine._h
    a, c = vbatches[5].inputs[False], tx_case
    g = Guarded([("bitmap", 8, 8), ("status", 8, 1), ("ids", 64, 1), ("tx_status", 8, 1), ("sig_status", 8, 1),
                 ("tx_ok", 8, 1), ("kind", 8, 1), ("left", 32, 4), ("right", 32, 4), ("node_hash", 64, 1),
                 ("tree_begin", 8, 4), ("pk", 32, 1), ("sig", 64, 1), ("words", 32, 4)], 0xA5)
    P = g.ptr
    vin = (_p(a["pk"]), _p(a["sig"]), _p(a["arena"]), _p(a["off"]), _p(a["len"]))
    t = ctypes.c_uint64(99)
    nn = ctypes.c_size_t(77)
    assert lib.cv_ed25519_verify_batch(h, 0, *vin, P("bitmap"), P("status")) == 0
    assert lib.cv_ed25519_verify_batch_ex(h, 0, *vin[:3], a["arena"].size, *vin[3:], P("bitmap"), P("status"), None) == 0
    assert lib.cv_ed25519_verify_batch_async(h, 0, *vin, P("bitmap"), P("status"), ctypes.byref(t)) == 0
    assert t.value == 0 and lib.cv_wait(h, t) == 0
    assert lib.cv_ed25519_verify_batch_keyed(h, 0, 1, _p(a["keys"]), _p(a["key_index"]), *vin[1:], P("bitmap"),
                                             P("status")) == 0
    lin = (_p(c["off"]), _p(c["len"]), _p(c["begin"]))
    assert lib.cv_merkle_tx_ids(h, 0, _p(c["arena"]), *lin, P("ids")) == 0
    assert lib.cv_merkle_tx_ids_ex(h, 0, _p(c["arena"]), *lin, P("ids"), P("tx_status")) == 0
    assert lib.cv_merkle_tx_ids_bounded(h, 0, _p(c["arena"]), c["arena"].size, *lin, P("ids"), P("tx_status"), None) == 0
    t.value = 99
    assert lib.cv_merkle_tx_ids_async(h, 0, _p(c["arena"]), *lin, P("ids"), P("tx_status"), ctypes.byref(t)) == 0
    assert t.value == 0
    tin = (*lin, _p(c["pk"]), _p(c["sig"]), _p(c["tsb"]), P("ids"), P("tx_status"), P("sig_status"), P("tx_ok"))
    assert lib.cv_verify_transactions(h, 0, _p(c["arena"]), *tin) == 0
    assert lib.cv_verify_transactions_ex(h, 0, _p(c["arena"]), c["arena"].size, *tin, None) == 0
    assert lib.cv_partial_merkle_verify(h, 0, 0, None, None, None, None, _p(c["begin"]), _p(c["ids"]), 0, None,
                                        _p(c["begin"]), P("tx_ok"), P("status")) == 0
    nodes = (P("kind"), P("left"), P("right"), P("node_hash"), P("tree_begin"), P("ids"), P("status"), ctypes.byref(nn))
    assert lib.cv_partial_merkle_build(h, 0, _p(c["ids"]), _p(c["begin"]), _p(c["ids"]), _p(c["begin"]), 1, *nodes) == 0
    assert lib.cv_filtered_build(h, 0, _p(c["arena"]), c["arena"].size, *lin, _p(c["st"]), 1, *nodes) == 0
    assert nn.value == 77
    assert lib.cv_ed25519_sign_batch(h, 0, _p(a["pk"]), _p(a["arena"]), _p(a["off"]), _p(a["len"]), P("pk"), P("sig")) == 0
    with native.Signer(engine, SIGNER_SEED) as s:
        assert lib.cv_ed25519_sign_keyed(h, s._h, 0, _p(a["arena"]), a["arena"].size, _p(a["off"]), _p(a["len"]),
                                         P("sig")) == 0
    with native.UniquenessSet(engine, 16) as u:
        assert lib.cv_uniq_commit_batch(u._h, 0, _p(c["ids"]), _p(c["begin"]), _p(c["ids"]), _p(c["begin"]), None,
                                        P("tx_status"), P("status"), P("ids"), P("words"), P("left")) == 0
        assert lib.cv_uniq_lookup(u._h, 0, _p(c["ids"]), P("status"), P("ids"), P("words"), P("left")) == 0
    for name in g.order:
        assert g.untouched(name), name
    g.check_guards("n == 0")


def test_bounded_calls_one_byte_short_touch_nothing(engine, vbatches, tx_case):
    """The CV_E_ARGS returns of the bounded calls with no ticket, the arena one byte short of what the records
    reach: no output byte is written."""
    lib, h = engine._lib, engine._h
    c = tx_case
    for n in (5, 65):
        b = vbatches[n]
        a = b.inputs[False]
        extent = int(lib.cv_msg_extent(n, _p(a["off"]), _p(a["len"])))
        g = _verify_outputs(engine, n, True, 0xA5, False)
        vin = (_p(a["pk"]), _p(a["sig"]), _p(a["arena"]))
        assert lib.cv_ed25519_verify_batch_ex(h, n, *vin, extent, _p(a["off"]), _p(a["len"]), g.ptr("bitmap"),
                                              g.ptr("status"), None) == 0
        g.refill()
        assert lib.cv_ed25519_verify_batch_ex(h, n, *vin, extent - 1, _p(a["off"]), _p(a["len"]), g.ptr("bitmap"),
                                              g.ptr("status"), None) == CV_E_ARGS
        assert g.untouched("bitmap") and g.untouched("status")
        g.check_guards(f"verify_batch_ex {n}")
    ntx, nsig = c["ntx"], c["nsig"]
    short = c["arena"].size - 1                        # the arena ends with the last leaf's last byte
    lin = (_p(c["off"]), _p(c["len"]), _p(c["begin"]))
    g = Guarded([("ids", 32 * ntx, 1), ("tx_status", ntx, 1), ("sig_status", nsig, 1), ("tx_ok", ntx, 1)], 0xA5)
    assert lib.cv_merkle_tx_ids_bounded(h, ntx, _p(c["arena"]), short, *lin, g.ptr("ids"), g.ptr("tx_status"),
                                        None) == CV_E_ARGS
    assert lib.cv_verify_transactions_ex(h, ntx, _p(c["arena"]), short, *lin, _p(c["pk"]), _p(c["sig"]), _p(c["tsb"]),
                                         g.ptr("ids"), g.ptr("tx_status"), g.ptr("sig_status"), g.ptr("tx_ok"),
                                         None) == CV_E_ARGS
    for name in g.order:
        assert g.untouched(name), name
    g.check_guards("bounded Merkle calls")


def _ascending_batch(corpus, n):
    """n corpus records whose messages are laid out one after another (a spare byte between them), so the offsets
    ascend and the LAST record reaches farthest: an arena one byte short fails in a call's last sub-chunk."""
    rows = corpus_rows(corpus, n, "accepted", seed=3)
    lens = _c(corpus["len"][rows], np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(lens[:-1].astype(np.uint64) + 1)
    arena = np.full(int(off[-1]) + int(lens[-1]), 0xEE, np.uint8)
    for o, l, s in zip(off, lens, corpus["off"][rows]):
        arena[int(o):int(o) + int(l)] = corpus["arena"][int(s):int(s) + int(l)]
    assert (off[:-1] + lens[:-1] < off[-1]).all()
    return dict(n=n, pk=_c(corpus["pk"][rows], np.uint8), sig=_c(corpus["sig"][rows], np.uint8), arena=arena, off=off,
                len=lens, verdict=corpus["verdict"][rows].astype(bool), status=corpus["status"][rows].astype(np.uint8))


def _verify_short_then_exact(eng, v, a, with_untouched, what):
    """cv_ed25519_verify_batch_ex with the arena one byte short (no ticket, then a ticket): CV_E_ARGS, ticket 0 and —
    with_untouched — no output byte written; then the whole arena: the batch's verdicts and status bytes."""
    lib, h, n = eng._lib, eng._h, v["n"]
    extent = int(lib.cv_msg_extent(n, _p(a["off"]), _p(a["len"])))
    assert extent == a["arena"].size == int(v["off"][-1]) + int(v["len"][-1])
    g = _verify_outputs(eng, n, True, 0xA5, False)

    def call(arena_bytes, ticket):
        return lib.cv_ed25519_verify_batch_ex(h, n, _p(a["pk"]), _p(a["sig"]), _p(a["arena"]), arena_bytes, _p(a["off"]),
                                              _p(a["len"]), g.ptr("bitmap"), g.ptr("status"), ticket)

    for with_ticket in (False, True):
        t = ctypes.c_uint64(99)
        assert call(extent - 1, ctypes.byref(t) if with_ticket else None) == CV_E_ARGS, (what, with_ticket)
        if with_ticket:
            assert t.value == 0, what
        if with_untouched:
            assert g.untouched("bitmap") and g.untouched("status"), (what, with_ticket)
        g.check_guards(f"{what} short, ticket={with_ticket}")
        g.refill()
        t = ctypes.c_uint64(0)
        assert call(extent, ctypes.byref(t) if with_ticket else None) == 0, (what, with_ticket)
        assert lib.cv_wait(h, t) == 0, what
        bm = g.read("bitmap", np.uint64)
        assert np.array_equal(native.bitmap_to_bools(bm, n), v["verdict"]), (what, with_ticket)
        assert tail_bits(bm, n) == 0, what
        assert np.array_equal(g.read("status"), v["status"]), (what, with_ticket)
        g.check_guards(f"{what} exact, ticket={with_ticket}")
        g.refill()


def test_bounded_calls_fail_inside_the_pipeline(engine, corpus, tx_case):
    """The CV_E_ARGS returns of the bounded calls from INSIDE the host pipeline (the one-byte-short test above only
    reaches the small paths): the arena one byte short of what the LAST record (leaf) reaches, and options under
    which the call has many sub-chunks, so the earlier ones are already enqueued when the last one is refused.  The
    call drains them, returns CV_E_ARGS with ticket 0 and writes no output byte; the same call with the whole arena
    then gives the exact results — the input ring, the staging blocks and the outputs were left usable.  Verify
    with and without a ticket, pageable and pinned arrays; Merkle ids and transactions in their asynchronous forms
    (at this size only those reach the pipeline); and the verify call cut over two virtual devices, where the shard
    that succeeded may have delivered its words, so only the return, the ticket and the next call are checked."""
    v = _ascending_batch(corpus, 1000)
    arrays = {k: v[k] for k in ("pk", "sig", "arena", "off", "len")}
    pipe = dict(pipe_min=64, pipe_first=64, pipe_chunk=128, auto_keyed=0)       # 1,000 records: >= 8 sub-chunks
    with Options(engine, **pipe):
        for pinned in (False, True):
            a = {k: engine.host_copy(x) for k, x in arrays.items()} if pinned else arrays
            _verify_short_then_exact(engine, v, a, True, f"verify pinned={pinned}")
    # ---- Merkle ids and transactions, asynchronous
    lib, h, c = engine._lib, engine._h, tx_case
    ntx, nsig = c["ntx"], c["nsig"]
    lin = (_p(c["off"]), _p(c["len"]), _p(c["begin"]))
    sizes = [("ids", 32 * ntx, 1), ("tx_status", ntx, 1), ("sig_status", nsig, 1), ("tx_ok", ntx, 1)]

    def merkle(g, arena_bytes, t):
        return lib.cv_merkle_tx_ids_bounded(h, ntx, _p(c["arena"]), arena_bytes, *lin, g.ptr("ids"), g.ptr("tx_status"),
                                            ctypes.byref(t))

    def txs(g, arena_bytes, t):
        return lib.cv_verify_transactions_ex(h, ntx, _p(c["arena"]), arena_bytes, *lin, _p(c["pk"]), _p(c["sig"]),
                                             _p(c["tsb"]), g.ptr("ids"), g.ptr("tx_status"), g.ptr("sig_status"),
                                             g.ptr("tx_ok"), ctypes.byref(t))

    with Options(engine, merkle_chunk=1, pipe_first=64, pipe_chunk=128):
        for name, call in (("merkle", merkle), ("transactions", txs)):
            g = Guarded(sizes, 0xA5)
            t = ctypes.c_uint64(99)
            assert call(g, c["arena"].size - 1, t) == CV_E_ARGS, name   # the arena ends with the last leaf's last byte
            assert t.value == 0, name
            for out in g.order:
                assert g.untouched(out), (name, out)
            g.check_guards(f"{name} short")
            t = ctypes.c_uint64(0)
            assert call(g, c["arena"].size, t) == 0, name
            assert lib.cv_wait(h, t) == 0, name
            assert np.array_equal(g.read("ids", shape=(ntx, 32)), c["ids"]), name
            assert np.array_equal(g.read("tx_status"), c["st"]), name
            if name == "transactions":
                assert np.array_equal(g.read("sig_status"), c["sst"]), name
                assert np.array_equal(g.read("tx_ok"), c["ok"]), name
            else:
                assert g.untouched("sig_status") and g.untouched("tx_ok")
            g.check_guards(f"{name} exact")
    # ---- the verify call cut over two virtual devices: the second shard holds the last record
    with native.Engine(1, virtual_devices=2) as e2:
        with Options(e2, shard_min=64, spread_min=64, **pipe):
            _verify_short_then_exact(e2, v, arrays, False, "verify, two virtual devices")
            assert e2.stats("route")["split_calls"] == 4                       # every call was cut over both
