"""The keyed verify path past its internal limits and across its chunk seams, on the GPU.

The keyed kernels (cv_keyprep_kernel, cv_keyed_prep_kernel, cv_comb_kernel<3>, cv_comb_quad_kernel,
cv_finish_kernel) with key_resolve and the key pool of cv_api.cpp, where their index arithmetic changes:

  A. more new keys in one call than one keyprep launch takes (kKeyprepBatch = 4,096), a pool that must grow to fit
     the call, a second call over the grown pool, in both comb forms;
  B. key lists with repeated rows, rows no signature references (invalid encodings among them), more keys than
     signatures, and every signature on the list's last row — through the host-buffer and the device-resident call;
  C. cv_ed25519_verify_device_keyed across the workspace-chunk seam (kVerifyChunk = 2^22 records);
  D. cv_ed25519_verify_device_timed, the call bench.py times, across the same seam.

Every expectation is exact: verdict bits, status bytes, tail bits, pool counters.  A mistake in any of these paths
keeps every access inside its buffer and gives wrong verdicts, which only a GPU run of the batched code shows (the
CPU harness runs one signature's key preparation and comb).
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from corda_amd import native  # noqa: E402

KEYPREP_BATCH = 4096                # kKeyprepBatch (cv_host.h): keys per keyprep launch
CHUNK = 1 << 22                     # kVerifyChunk (cv_host.h): records per workspace chunk
SEAM_N = CHUNK + 200_003            # two workspace chunks, the second one ragged (as test_split_launch_plans_agree)


def _bits(bitmap, n):
    return native.bitmap_to_bools(bitmap, n)


def _tail_clear(bitmap, n):
    return n % 64 == 0 or int(bitmap[-1]) >> (n % 64) == 0


def _stats_delta(after, before):
    return {k: after[k] - before[k] for k in ("hits", "misses")}


# ---------------------------------------------------------------- A: more than 4,096 new keys in one call
NK1 = 2 * KEYPREP_BATCH + 5         # keys of the first call: three keyprep launches (4,096 + 4,096 + 5)
NEW2 = KEYPREP_BATCH + 404          # brand-new keys of the second call (4,500: two keyprep launches)
OLD2 = 3000                         # keys the second call shares with the first
SECOND = 600                        # keys with a second signature in the first call


@pytest.fixture(scope="module")
def limits(engine, oracle_c):
    """NK1 + NEW2 distinct keys with one signature each (messages of 0-120 bytes at contiguous offsets), a second
    signature for the first 600; every 7th signature with a low S bit flipped, every 11th key row and the rows
    around each keyprep batch boundary of both calls with a byte flipped (their signatures left alone).  The two
    calls' records with the C oracle's verdicts and statuses, computed once."""
    rng = np.random.default_rng(20261020)
    kt = NK1 + NEW2
    rec_key = np.concatenate([np.arange(kt), np.arange(SECOND)])          # record -> key
    nrec = rec_key.size
    seeds = rng.integers(0, 256, (kt, 32), dtype=np.uint8)
    ln = rng.integers(0, 121, nrec).astype(np.uint32)
    off = np.zeros(nrec, np.uint64)
    off[1:] = np.cumsum(ln[:-1])
    arena = rng.integers(0, 256, int(ln.sum()) + 16, dtype=np.uint8)
    pk, sig = engine.sign_batch(seeds[rec_key], arena, off, ln)
    keys = pk[:kt].copy()
    assert len({bytes(r) for r in keys}) == kt
    sig[::7, 32] ^= 0x01                                                   # low bit of S
    # the second call's new keys are its list rows OLD2.., so its keyprep batch boundary is key NK1 + 4,096
    forced = [b + d for b in (KEYPREP_BATCH, 2 * KEYPREP_BATCH, NK1 + KEYPREP_BATCH) for d in range(-2, 3)]
    assert forced[:5] == [4094, 4095, 4096, 4097, 4098] and forced[5:10] == [8190, 8191, 8192, 8193, 8194]
    for r in sorted(set(range(0, kt, 11)) | set(forced)):
        keys[r, (r // 11) % 32] ^= 0x20                                    # a non-point or another point
    assert len({bytes(r) for r in keys}) == kt
    sel1 = np.concatenate([np.arange(NK1), kt + np.arange(SECOND)])
    sel2 = np.arange(NK1 - OLD2, kt)
    calls = []
    for sel, k0, k1 in ((sel1, 0, NK1), (sel2, NK1 - OLD2, kt)):
        kidx = (rec_key[sel] - k0).astype(np.uint32)
        klist = np.ascontiguousarray(keys[k0:k1])
        ref, rst = oracle_c.verify_batch(klist[kidx], sig[sel], arena, off[sel], ln[sel], nthreads=8)
        # non-vacuity, on the oracle's own array: the strides above leave about 0.78 accepted
        assert 0.5 < ref.mean() < 0.95
        assert 0 < int((rst != 0).sum()) < sel.size
        calls.append(dict(keys=klist, kidx=kidx, sig=np.ascontiguousarray(sig[sel]), off=off[sel], ln=ln[sel],
                          verdict=ref.astype(bool), status=rst))
    return dict(arena=arena, calls=calls)


def _call(e, d, k):
    c = d["calls"][k]
    bitmap, status = e.verify_batch_keyed(c["keys"], c["kidx"], c["sig"], d["arena"], c["off"], c["ln"])
    n = c["kidx"].size
    bad = np.where(_bits(bitmap, n) != c["verdict"])[0]
    assert bad.size == 0, (f"call {k}: {bad.size} verdicts differ from the oracle, first at records {bad[:8]} "
                           f"(keys {c['kidx'][bad[:8]]})")
    bad = np.where(status != c["status"])[0]
    assert bad.size == 0, f"call {k}: {bad.size} status bytes differ, first at keys {c['kidx'][bad[:8]]}"
    assert _tail_clear(bitmap, n)


@pytest.mark.parametrize("quad_max", [None, 0], ids=["comb_quad", "comb3"])
def test_keyprep_batches_and_pool_growth(limits, quad_max):
    """8,197 new keys in one host keyed call on a pool reserved for 64: key_resolve grows the pool to fit and
    builds the tables in three keyprep launches (offsets miss_keys + 32 k0, miss_slots + k0); verdicts and statuses
    equal the C oracle's, resident = misses = the keys.  A second call (the last 3,000 of those keys, then 4,500 new
    ones: two more launches) either fits or empties the pool first, and is exact either way.  Under quad_max = 0
    (cv_comb_kernel<3> in place of cv_comb_quad_kernel) the first call runs again on a fresh engine, so both comb
    forms read tables of later keyprep launches."""
    e = native.Engine(1)
    try:
        e.key_cache_reserve(64)
        if quad_max is not None:
            e.set_option("quad_max", quad_max)
        s0 = e.key_cache_stats(0)
        assert s0["resident"] == 0
        _call(e, limits, 0)
        s1 = e.key_cache_stats(0)
        assert s1["resident"] == NK1
        assert s1["capacity"] >= NK1
        assert s1["misses"] - s0["misses"] == NK1
        assert s1["hits"] - s0["hits"] == 0
        if quad_max is not None:
            return
        _call(e, limits, 1)
        s2 = e.key_cache_stats(0)
        # the engine counts no resets in cv_key_cache_stats, but the resident count tells: an emptied pool holds
        # this call's keys only and every one of them missed; otherwise the 3,000 old keys hit
        n2 = OLD2 + NEW2
        assert (s2["resident"], s2["misses"] - s1["misses"], s2["hits"] - s1["hits"]) in \
            {(n2, n2, 0), (NK1 + NEW2, NEW2, OLD2)}
        assert s2["capacity"] >= s2["resident"]
    finally:
        e.close()


def test_hits_and_misses_across_keyprep_batches(limits):
    """The same two calls on a pool of the default capacity (16,384 keys), which holds both: the second call's 3,000
    old keys hit the slots of the first call's later keyprep launches, its 4,500 new ones take slots 8,197.. in two
    launches (slot numbers that differ from the launch's own row numbers), nothing is emptied."""
    e = native.Engine(1)
    try:
        _call(e, limits, 0)
        s1 = e.key_cache_stats(0)
        assert s1["capacity"] >= NK1 + NEW2, "the default pool no longer holds both calls: reserve it here"
        _call(e, limits, 1)
        s2 = e.key_cache_stats(0)
        assert s2["resident"] == NK1 + NEW2
        assert _stats_delta(s2, s1) == {"hits": OLD2, "misses": NEW2}
    finally:
        e.close()


# ---------------------------------------------------------------- B: untidy key lists
def _run_keyed(e, api, keys, kidx, sig, arena, off, ln):
    """One keyed call through the host-buffer entry point or the device-resident one (outputs prefilled with ones
    and 7s there) -> (bitmap u64, status u8)."""
    if api == "host":
        return e.verify_batch_keyed(keys, kidx, sig, arena, off, ln)
    import torch
    dev = "cuda:0"
    n = len(kidx)

    def up(a, view=None):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(view) if view else a).to(dev)

    t = [up(keys), up(np.asarray(kidx, np.uint32), np.int32), up(sig),
         up(np.concatenate([np.asarray(arena, np.uint8), np.zeros(64, np.uint8)])),
         up(np.asarray(off, np.uint64), np.int64), up(np.asarray(ln, np.uint32), np.int32)]
    bm = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=dev)
    st = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    e.verify_device_keyed(0, n, len(keys), *[x.data_ptr() for x in t], bm.data_ptr(), st.data_ptr())
    e.synchronize(0)
    return bm.cpu().numpy().view(np.uint64), st.cpu().numpy()


def _untidy(corpus):
    """The corpus's 324 distinct keys (invalid, non-canonical and small-order ones among them), every key a second
    time in reverse order, then 40 rows no signature references (20 of random bytes, 20 of 0xFF); each signature's
    key_index alternately on the first and the second copy of its key."""
    keys0, inv = np.unique(corpus["pk"], axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    k = len(keys0)
    rng = np.random.default_rng(324)
    keys = np.concatenate([keys0, keys0[::-1], rng.integers(0, 256, (20, 32), dtype=np.uint8),
                           np.full((20, 32), 0xFF, np.uint8)])
    i = np.arange(len(inv))
    kidx = np.where(i % 2 == 0, inv, 2 * k - 1 - inv).astype(np.uint32)
    assert np.array_equal(keys[kidx], corpus["pk"])
    assert (kidx < k).any() and (kidx >= k).any()
    return np.ascontiguousarray(keys), kidx


def _lookups(api, keys, kidx):
    """(rows the call looks up, distinct keys among them): the device-resident call resolves every row of its key
    list; the host-buffer call only the rows some signature references (include/cordaverify.h, cv_key_cache_stats)."""
    rows = np.arange(len(keys)) if api == "device" else np.unique(kidx)
    return len(rows), len({bytes(keys[r]) for r in rows})


def _cold_and_warm(api, keys, kidx, sig, arena, off, ln, verdict, status):
    """The call twice on an engine of its own.  Cold: each distinct key looked up misses once, the further rows that
    repeat it hit (the choice pinned here: hits + misses = rows looked up), resident = the distinct keys.  Warm: every
    row hits, nothing is recomputed.  (The miss count is what notices a repeated key taking a second slot and a
    second table build: the resident count is the size of a map keyed by the key bytes and stays the same.)"""
    rows, distinct = _lookups(api, keys, kidx)
    n = len(kidx)
    e = native.Engine(1)
    try:
        # room for the resident keys plus every row of the warm call: key_resolve empties the pool when those two
        # together pass the capacity, whether or not the rows are resident already
        e.key_cache_reserve(2048)
        assert distinct + rows <= 2048
        before = e.key_cache_stats(0)
        for rep, want in (("cold", {"hits": rows - distinct, "misses": distinct}), ("warm", {"hits": rows, "misses": 0})):
            bitmap, st = _run_keyed(e, api, keys, kidx, sig, arena, off, ln)
            bad = np.where(_bits(bitmap, n) != verdict.astype(bool))[0]
            assert bad.size == 0, f"{api} {rep}: verdicts differ at records {bad[:8]} (key rows {kidx[bad[:8]]})"
            assert np.array_equal(st, status), f"{api} {rep}: status"
            assert bitmap.size == (n + 63) // 64 and _tail_clear(bitmap, n), f"{api} {rep}: tail bits"
            after = e.key_cache_stats(0)
            assert after["resident"] == distinct, f"{api} {rep}: resident keys"
            assert _stats_delta(after, before) == want, f"{api} {rep}"
            before = after
    finally:
        e.close()
    return rows, distinct


@pytest.mark.parametrize("api", ["host", "device"])
def test_duplicate_and_unreferenced_key_rows(corpus, api):
    """Repeated rows (the fresh.find branch of key_resolve) and unreferenced rows: the corpus's pinned verdicts and
    statuses, and resident = the distinct key byte strings — of the whole list through the device-resident call
    (which builds tables for the unreferenced rows too, invalid encodings among them), of the referenced rows
    through the host-buffer call (which never reads the others)."""
    keys, kidx = _untidy(corpus)
    rows, distinct = _cold_and_warm(api, keys, kidx, corpus["sig"], corpus["arena"], corpus["off"], corpus["len"],
                                    corpus["verdict"], corpus["status"])
    if api == "device":
        assert (rows, distinct) == (len(keys), len({bytes(r) for r in keys}))
        assert distinct == 324 + 20, "0xFF x 32 is one of the corpus's keys; the random rows are new"
    else:
        assert distinct == 324 and 324 < rows <= 648


@pytest.mark.parametrize("api", ["host", "device"])
def test_more_keys_than_signatures(corpus, api):
    """nkeys > n: the same 688-row list with the first 10 signatures only."""
    keys, kidx = _untidy(corpus)
    n = 10
    assert len(keys) > n
    _cold_and_warm(api, keys, kidx[:n], corpus["sig"][:n], corpus["arena"], corpus["off"][:n], corpus["len"][:n],
                   corpus["verdict"][:n], corpus["status"][:n])


@pytest.mark.parametrize("api", ["host", "device"])
def test_every_signature_on_the_last_key_row(engine, corpus, oracle_c, api):
    """Every key_index = nkeys - 1: one honest key after the untidy list, 200 honest signatures from it and 20 with
    a flipped S bit."""
    keys, _ = _untidy(corpus)
    rng = np.random.default_rng(220)
    n = 220
    seed = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    ln = rng.integers(0, 121, n).astype(np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1])
    arena = rng.integers(0, 256, int(ln.sum()) + 16, dtype=np.uint8)
    pk, sig = engine.sign_batch(np.repeat(seed, n, axis=0), arena, off, ln)
    assert (pk == pk[0]).all()
    keys = np.ascontiguousarray(np.concatenate([keys, pk[:1]]))
    kidx = np.full(n, len(keys) - 1, np.uint32)
    sig[5::11, 32] ^= 0x01
    ref, rst = oracle_c.verify_batch(keys[kidx], sig, arena, off, ln, nthreads=4)
    assert int(ref.sum()) == 200 and not ref[5::11].any() and int(rst.sum()) == 0
    rows, distinct = _cold_and_warm(api, keys, kidx, sig, arena, off, ln, ref, rst)
    if api == "host":
        assert (rows, distinct) == (1, 1)


# ---------------------------------------------------------------- C, D: across the 2^22 workspace-chunk seam
@pytest.fixture(scope="module")
def seam(corpus):
    """The golden corpus tiled by a seeded random index to 2^22 + 200,003 records on the device, as
    test_split_launch_plans_agree builds them, with the corpus's distinct keys and each record's index into them;
    uploaded once for the tests below."""
    import torch
    n = SEAM_N
    rng = np.random.default_rng(7)
    idx = rng.integers(0, len(corpus["pk"]), n)
    keys, inv = np.unique(corpus["pk"], axis=0, return_inverse=True)
    inv = inv.reshape(-1).astype(np.uint32)
    assert np.array_equal(keys[inv], corpus["pk"])
    dev = "cuda:0"
    d = dict(n=n, nkeys=len(keys), verdict=corpus["verdict"][idx].astype(bool), status=corpus["status"][idx])
    d["keys"] = torch.from_numpy(np.ascontiguousarray(keys)).to(dev)
    d["kidx"] = torch.from_numpy(np.ascontiguousarray(inv[idx]).view(np.int32)).to(dev)
    d["pk"] = torch.from_numpy(np.ascontiguousarray(corpus["pk"][idx])).to(dev)
    d["sig"] = torch.from_numpy(np.ascontiguousarray(corpus["sig"][idx])).to(dev)
    d["arena"] = torch.from_numpy(np.concatenate([corpus["arena"], np.zeros(64, np.uint8)])).to(dev)
    d["off"] = torch.from_numpy(corpus["off"][idx].astype(np.uint64).view(np.int64)).to(dev)
    d["len"] = torch.from_numpy(corpus["len"][idx].astype(np.uint32).view(np.int32)).to(dev)
    torch.cuda.synchronize()
    yield d
    d.clear()
    torch.cuda.empty_cache()


def _seam_moves(d):
    """The expected verdicts around record 2^22 are not invariant under a shift by 1, 8 or 64 records (nor by a
    whole chunk), so a pointer that fails to advance at the seam cannot give them; with a mean of 0.53 they are
    not, whatever the seed."""
    v = d["verdict"]
    lo, hi = CHUNK - 128, CHUNK + 128
    for s in (1, 8, 64):
        assert not np.array_equal(v[lo:hi], v[lo + s:hi + s]) and not np.array_equal(v[lo:hi], v[lo - s:hi - s])
    assert not np.array_equal(v[CHUNK:CHUNK + 128], v[:128])
    assert 0 < int((d["status"][lo:hi] != 0).sum()) < hi - lo
    assert not np.array_equal(d["status"][CHUNK:CHUNK + 128], d["status"][:128])


def _check_seam_bitmap(d, bits, what):
    n = d["n"]
    assert bits.size == (n + 63) // 64
    want = np.packbits(d["verdict"], bitorder="little")
    want = np.concatenate([want, np.zeros(bits.size * 8 - want.size, np.uint8)]).view(np.uint64)
    w = CHUNK // 64
    for k in (w - 1, w):                        # the words just before and just after the seam
        assert int(bits[k]) == int(want[k]), f"{what}: bitmap word {k} at the chunk seam"
    bad = np.where(_bits(bits, n) != d["verdict"])[0]
    assert bad.size == 0, f"{what}: {bad.size} verdicts differ, first at records {bad[:8]}"
    assert int(bits[-1]) >> (n % 64) == 0, f"{what}: bits past n"
    assert np.array_equal(bits, want)


@pytest.mark.parametrize("want_status", [True, False], ids=["status", "no_status"])
def test_keyed_device_across_workspace_chunks(engine, seam, want_status):
    """cv_ed25519_verify_device_keyed at 2^22 + 200,003 records: cvk_verify_keyed runs two workspace chunks
    (key_index + c0, sig + 64 c0, status + c0, the finish kernel's bitmap + c0 / 8), over a bitmap of ones and a
    status array of 7s: every verdict bit and status byte follows its record, the bits past n are clear, the words
    and bytes on both sides of record 2^22 are right.  Once with a status pointer and once without."""
    import torch
    d = seam
    n = d["n"]
    assert math.ceil(n / CHUNK) == 2 and n % 64
    _seam_moves(d)
    bm = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda:0")
    st = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    engine.verify_device_keyed(0, n, d["nkeys"], d["keys"].data_ptr(), d["kidx"].data_ptr(), d["sig"].data_ptr(),
                               d["arena"].data_ptr(), d["off"].data_ptr(), d["len"].data_ptr(), bm.data_ptr(),
                               st.data_ptr() if want_status else 0)
    engine.synchronize(0)
    _check_seam_bitmap(d, bm.cpu().numpy().view(np.uint64), "keyed device")
    got = st.cpu().numpy()
    if want_status:
        for i in (CHUNK - 1, CHUNK):
            assert got[i] == d["status"][i], f"status byte {i} at the chunk seam"
        assert np.array_equal(got, d["status"])
    else:
        assert (got == 7).all(), "status written without a status pointer"


def test_timed_device_across_verify_chunks(engine, seam):
    """cv_ed25519_verify_device_timed (what bench.py times) at 2^22 + 200,003 records: its own loop over 2^22-record
    chunks (d_pk + 32 c0 .. d_bitmap + c0 / 64, phase times summed) gives the bitmap cv_ed25519_verify_device gives
    for the same inputs and the corpus's pinned verdicts; three finite, non-negative phase times with a positive
    sum."""
    import torch
    d = seam
    n = d["n"]
    _seam_moves(d)
    args = [d[k].data_ptr() for k in ("pk", "sig", "arena", "off", "len")]
    bm_t = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda:0")
    bm_p = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ms = engine.verify_device_timed(0, n, *args, bm_t.data_ptr())
    engine.verify_device(0, n, *args, bm_p.data_ptr())
    engine.synchronize(0)
    timed = bm_t.cpu().numpy().view(np.uint64)
    _check_seam_bitmap(d, timed, "timed")
    assert np.array_equal(timed, bm_p.cpu().numpy().view(np.uint64)), "timed and plain device verify differ"
    assert len(ms) == 3 and all(math.isfinite(x) and x >= 0 for x in ms), ms
    assert sum(ms) > 0, ms
