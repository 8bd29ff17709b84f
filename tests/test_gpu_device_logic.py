"""The product's device-only code on the GPU itself, value by value: tests/device_harness.hip puts the field forms
(the v_mad_u64_u32 columns of cv_madc.h), the lattice (the hardware reciprocal in cv_qdiv), the hashes' device
variants, the decodes and tables, and the DPP quad formulas of cv_quad.h / cv_hsquad.h behind small kernels, and
every output is compared by exact integer equality with Python big integers, hashlib or oracle/ed25519_ref.py.
The vectors are those of the CPU layer (test_device_logic.py, through device_vectors.py).

What this does not cover: the production kernels are separate compilations with their own launch bounds, so their
code generation is still checked only at the verdict level (test_gpu_parity.py, test_gpu_torsion_maxlimb.py)."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

import device_harness_build
import device_vectors as V
import ed25519_ref as E

P, L, D2 = E.P, E.L, E.D2
gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIDTH = np.array(V.W)
TIGHT = np.array([int(1.01 * (1 << w)) for w in V.W], np.int64)          # cv_field.h: "tight" <= 1.01 * 2^w_i
UNIT = np.array([1 << w for w in V.W], np.int64)
KP = lambda k: np.array([k * 0x3ffffed] + [k * 0x1ffffff, k * 0x3ffffff] * 4 + [k * 0x1ffffff], np.int64)  # noqa: E731
LANES = 4096                                                             # lanes per launch, at most


def test_device_harness_compiles_for_gfx950():
    """No GPU needed: a header change that breaks the harness shows up on the CPU suite.  Builds (or finds up to
    date) tests/_build/libcvdev.so and does not load it."""
    lib = device_harness_build.build()
    assert os.path.getsize(lib) > 100_000


class Dev:
    """ctypes front of libcvdev.so.  A non-zero return fails the test with that code, and after a HIP error nothing
    more is launched: every later call fails at once."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.dead = None

    def run(self, name, inp, outw, pre=(), post=(), per=1):
        """inp: (items, words) uint32; launches of at most LANES lanes (per = lanes per item); returns (items, outw)."""
        if self.dead:
            pytest.fail(f"not run: {self.dead}")
        inp = np.ascontiguousarray(inp, np.uint32)
        n = inp.shape[0]
        out = np.zeros((n, outw), np.uint32)
        vp = ctypes.c_void_p
        step = LANES // per
        for lo in range(0, n, step):
            a, o = inp[lo:lo + step], out[lo:lo + step]
            rc = getattr(self.lib, name)(*pre, ctypes.c_uint32(a.shape[0]), a.ctypes.data_as(vp), o.ctypes.data_as(vp),
                                         *post)
            if rc > 0:
                self.dead = f"{name} returned hipError_t {rc}"
            if rc != 0:
                pytest.fail(f"{name} returned {rc}")
        return out

    def quad(self, name, seq, inp, outw, pre=(), post=()):
        """Four lanes per item, whole waves: pads to a multiple of 16 items by repeating the last one."""
        inp = np.ascontiguousarray(inp, np.uint32)
        n = inp.shape[0]
        pad = (-n) % 16
        if pad:
            inp = np.concatenate([inp, np.repeat(inp[-1:], pad, axis=0)])
        return self.run(name + ("_seq" if seq else "_ilp"), inp, outw, pre, post, per=4)[:n]


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Dev(device_harness_build.build())


# ---------------------------------------------------------------- helpers
def to_limbs(v):
    return [(v >> o) & ((1 << w) - 1) for o, w in zip(V.OFF, V.W)]


def vals(a):
    """Rows of ten limbs -> Python integers."""
    return [V.limb_val(r) for r in np.asarray(a).reshape(-1, 10).tolist()]


def words(v, n=8):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def from_words(a):
    return [sum(int(x) << (32 * i) for i, x in enumerate(r)) for r in np.asarray(a).tolist()]


def assert_tight(a, what):
    a = np.asarray(a, np.int64).reshape(-1, 10)
    bad = np.nonzero((a > TIGHT).any(axis=1))[0]
    assert bad.size == 0, f"{what}: limbs above 1.01 * 2^w in {bad.size} outputs, first {a[bad[0]].tolist()}"


def assert_vals(out, want, what):
    got = vals(out)
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if (g - w) % P]
    assert not bad, f"{what}: {len(bad)} wrong values, first at vector {bad[0]}"


def field_vectors(rng, mult_f, mult_g, n=2000):
    """(f, g) limb vectors: n drawn at the bounds, the all-maximum pair, and test_field_ops_random_and_extreme's
    values (canonical limbs) paired among themselves."""
    fs = [V.limbs(rng, mult_f) for _ in range(n)] + [V.max_limbs(mult_f)]
    gs = [V.limbs(rng, mult_g) for _ in range(n)] + [V.max_limbs(mult_g)]
    fv = V.field_values(random.Random(1))
    fs += [to_limbs(a) for a in fv]
    gs += [to_limbs(rng.choice(fv)) for _ in fv]
    return fs, gs


# ---------------------------------------------------------------- field
@gpu
def test_field_products(dev):
    """fe_mul, fe_mul_ilp and fe_mul_n<2, 3, 4> at f <= 8 M_i, g <= 3.3 M_i: value mod p and tight output limbs."""
    rng = random.Random(2)
    for form, name in ((0, "fe_mul"), (1, "fe_mul_ilp")):
        fs, gs = field_vectors(rng, 8.0, 3.29)
        out = dev.run("cvd_fe_mul", np.hstack([fs, gs]), 10, pre=(form,))
        assert_vals(out, [V.limb_val(f) * V.limb_val(g) for f, g in zip(fs, gs)], name)
        assert_tight(out, name)
    for nch in (2, 3, 4):
        cols = [field_vectors(rng, 8.0, 3.29) for _ in range(nch)]
        inp = np.hstack([c[0] for c in cols] + [c[1] for c in cols])
        out = dev.run("cvd_fe_mul_n", inp, 10 * nch, pre=(nch,))
        for m, (fs, gs) in enumerate(cols):
            assert_vals(out[:, 10 * m:10 * m + 10], [V.limb_val(f) * V.limb_val(g) for f, g in zip(fs, gs)],
                        f"fe_mul_n<{nch}> chain {m}")
        assert_tight(out, f"fe_mul_n<{nch}>")


@gpu
def test_field_squares(dev):
    """fe_sq, fe_sq2, fe_sq_rt, fe_sq_ilp (both doubling flags), fe_sq_n<2, 0> and fe_sq_n<4, 0x4> at f <= 3.3 M_i."""
    rng = random.Random(12)
    for form, flag, name in ((0, 0, "fe_sq"), (1, 0, "fe_sq2"), (2, 0, "fe_sq_rt(0)"), (2, 1, "fe_sq_rt(1)"),
                             (3, 0, "fe_sq_ilp(0)"), (3, 1, "fe_sq_ilp(1)")):
        fs, _ = field_vectors(rng, 3.29, 3.29)
        inp = np.hstack([fs, np.full((len(fs), 1), flag)])
        out = dev.run("cvd_fe_sq", inp, 10, pre=(form,))
        k = 2 if (form == 1 or flag) else 1
        assert_vals(out, [k * V.limb_val(f) ** 2 for f in fs], name)
        assert_tight(out, name)
    for nch, dbl in ((2, 0), (4, 0x4)):
        cols = [field_vectors(rng, 3.29, 3.29)[0] for _ in range(nch)]
        out = dev.run("cvd_fe_sq_n", np.hstack(cols), 10 * nch, pre=(nch,))
        for m, fs in enumerate(cols):
            k = 2 if (dbl >> m) & 1 else 1
            assert_vals(out[:, 10 * m:10 * m + 10], [k * V.limb_val(f) ** 2 for f in fs], f"fe_sq_n<{nch}> chain {m}")
        assert_tight(out, f"fe_sq_n<{nch}, {dbl}>")


@gpu
def test_field_linear_and_conversions(dev):
    """fe_sub<2, 3, 4>, fe_sub_carry_even<3>, fe_carry, fe_carry_even, fe_neg, fe_from_words, fe_to_words."""
    rng = random.Random(21)
    for form, k, name in ((0, 2, "fe_sub<2>"), (1, 3, "fe_sub<3>"), (2, 4, "fe_sub<4>"), (3, 3, "fe_sub_carry_even<3>")):
        # subtrahend limbs g_i <= k p_i (the precondition: |k p_i - g_i| + f_i equals f + k p - g only then), at and
        # below that edge; f up to 8 units
        kp = KP(k)
        fs, _ = field_vectors(rng, 8.0, 1.0)
        gs = np.array([[rng.choice([int(kp[i]), int(kp[i]) - 1, rng.randrange(int(kp[i]) + 1), 0]) for i in range(10)]
                       for _ in fs], np.int64)
        gs[0] = kp
        assert (gs <= kp).all()
        f = np.array(fs, np.int64)
        out = dev.run("cvd_fe_sub", np.hstack([f, gs]), 10, pre=(form,)).astype(np.int64)
        assert_vals(out, [V.limb_val(a) - V.limb_val(b) for a, b in zip(fs, gs.tolist())], name)
        if form < 3:
            assert (out <= f + k * UNIT).all(), name                       # result <= f + k, in units of M_i
            assert (out == f + kp - gs).all(), name
        else:
            assert (out[:, 0::2] < (1 << 26)).all(), name                  # even limbs carried
            assert (out[:, 1::2] <= f[:, 1::2] + k * UNIT[1::2] + ((f[:, 0::2] + k * UNIT[0::2]) >> 26)).all(), name
    wide = [V.limbs(rng, 31.99) for _ in range(2000)] + [[(1 << 31) - 1] * 10] + [V.max_limbs(8.0)]    # limbs < 2^31
    out = dev.run("cvd_fe_un", wide, 10, pre=(0,))
    assert_vals(out, [V.limb_val(f) for f in wide], "fe_carry")
    assert_tight(out, "fe_carry")
    out = dev.run("cvd_fe_un", wide, 10, pre=(1,)).astype(np.int64)
    assert_vals(out, [V.limb_val(f) for f in wide], "fe_carry_even")
    w = np.array(wide, np.int64)
    assert (out[:, 0::2] < (1 << 26)).all() and (out[:, 1::2] == w[:, 1::2] + (w[:, 0::2] >> 26)).all()
    tight = [V.limbs(rng, 1.0099) for _ in range(2000)] + [TIGHT.tolist(), KP(2).tolist(), [0] * 10]
    out = dev.run("cvd_fe_un", tight, 10, pre=(2,)).astype(np.int64)
    assert_vals(out, [-V.limb_val(f) for f in tight], "fe_neg")
    assert (out <= KP(2)).all()
    # fe_from_words (bit 255 ignored, not reduced, limbs < M_i) and fe_to_words (canonical, limbs < 2^31 in)
    raw = V.field_values(random.Random(1)) + [rng.getrandbits(256) for _ in range(2000)] + [2**256 - 1, 2**255, 2**255 + P]
    wide = wide[:len(raw)] + [V.limbs(rng, 31.99) for _ in range(len(raw) - len(wide))]
    out = dev.run("cvd_fe_words", np.hstack([[words(v) for v in raw], wide[:len(raw)]]), 18)
    assert vals(out[:, :10]) == [v & ((1 << 255) - 1) for v in raw]
    assert (out[:, :10].astype(np.int64) < UNIT).all()
    assert from_words(out[:, 10:]) == [V.limb_val(f) % P for f in wide[:len(raw)]]


@gpu
def test_field_powers(dev):
    """fe_invert<false / true> (z^(p-2)) and fe_pow22523<false / true> (z^(2^252-3)) over inputs up to 3.3 M_i."""
    rng = random.Random(23)
    for form, e, name in ((3, P - 2, "fe_invert<false>"), (4, P - 2, "fe_invert<true>"),
                          (5, (P - 5) // 8, "fe_pow22523<false>"), (6, (P - 5) // 8, "fe_pow22523<true>")):
        fs, _ = field_vectors(rng, 3.29, 3.29)
        out = dev.run("cvd_fe_un", fs, 10, pre=(form,))
        assert_vals(out, [pow(V.limb_val(f) % P, e, P) for f in fs], name)
        assert_tight(out, name)


# ---------------------------------------------------------------- scalars
@gpu
def test_scalar_reduce_and_muladd(dev):
    cases = V.sc_reduce_cases(random.Random(3))
    out = dev.run("cvd_sc_reduce", [words(int.from_bytes(x, "little"), 16) for x in cases], 8)
    assert from_words(out) == [int.from_bytes(x, "little") % L for x in cases]
    rng = random.Random(4)
    abc = [tuple(rng.getrandbits(256) for _ in range(3)) for _ in range(500)]
    abc += [(2**256 - 1,) * 3, (L - 1, L - 1, L - 1), (0, 0, 0), (L, L, L), (2**255, 2**255 + 1, 2**256 - 1)]
    out = dev.run("cvd_sc_muladd", [words(a) + words(b) + words(c) for a, b, c in abc], 8)
    assert from_words(out) == [(a * b + c) % L for a, b, c in abc]


@gpu
def test_exact_quotient_with_hardware_reciprocal(dev):
    """cv_exact_quotient + cv_submul8 with the device's cv_qdiv (v_rcp_f64 + two Newton steps) on the host test's
    ~20 k pairs: 1 <= q <= floor(r0 / r1) (the remainder never wraps), remainder = r0 - q r1, and q at most one
    short of the true quotient where that is below 2^32."""
    cases = V.exact_step_cases(random.Random(99))
    assert len(cases) > 15000
    out = dev.run("cvd_exact_step", [words(r0) + words(r1) for r0, r1 in cases], 9)
    qs, rems = out[:, 0].tolist(), from_words(out[:, 1:])
    bad = []
    for (r0, r1), q, rem in zip(cases, qs, rems):
        true_q = r0 // r1
        ok = 1 <= q <= true_q and rem == r0 - q * r1
        if true_q < 2 ** 32:
            ok = ok and true_q - q <= 1 and rem < 2 * r1
        if not ok:
            bad.append((r0, r1, q, true_q))
    assert not bad, (len(bad), bad[:3])


def _halfsize(dev, cases):
    out = dev.run("cvd_halfsize", [words(h) + words(s) for h, s in cases], 27)
    u, va, w = from_words(out[:, 0:8]), from_words(out[:, 8:16]), from_words(out[:, 16:24])
    return u, va, w, out[:, 24].tolist(), out[:, 25].tolist(), out[:, 26].tolist()


@gpu
def test_halfsize_lattice_with_hardware_reciprocal(dev, host_harness):
    """sc_halfsize on the device, the host test's 3,007 cases and every property it asserts: v odd, u = v h (mod 8L),
    w = -v s (mod L), |u|, |v| < 16^nwin, fallback (h, 1, 64 windows) only among the seven edge cases.  The number of
    cases whose (u, v, w, nwin) differ from the host's exact-division run is reported, not asserted: another valid
    short vector is allowed, the properties are the contract."""
    cases = V.halfsize_cases(random.Random(7))
    assert len(cases) == 3007
    u, va, w, vneg, nwin, ok = _halfsize(dev, cases)
    H = host_harness
    H.cvh_set_rcp_emulation.argtypes = [ctypes.c_double]
    H.cvh_set_rcp_emulation(0.0)
    wins, fallbacks, differ = [], 0, 0
    for ci, (h, s) in enumerate(cases):
        v = -va[ci] if vneg[ci] else va[ci]
        assert v % 2 == 1, ci
        assert (u[ci] - v * h) % (8 * L) == 0, ci
        assert w[ci] == (-v * s) % L, ci
        assert u[ci] >= 0 and max(u[ci], va[ci]) < 16 ** nwin[ci], ci
        if ok[ci]:
            assert nwin[ci] <= 36
            wins.append(nwin[ci])
        else:
            fallbacks += 1
            assert ci < V.HALFSIZE_EDGES, "fallback on a random scalar"
            assert (u[ci], v, nwin[ci]) == (h, 1, 64)
        o = (ctypes.c_uint8 * 96)()
        vn, nw = ctypes.c_int(0), ctypes.c_int(0)
        H.cvh_halfsize(h.to_bytes(32, "little"), s.to_bytes(32, "little"), o, ctypes.byref(vn), ctypes.byref(nw))
        hb = bytes(o)
        host = tuple(int.from_bytes(hb[32 * k:32 * k + 32], "little") for k in range(3)) + (vn.value, nw.value)
        differ += host != (u[ci], va[ci], w[ci], vneg[ci], nwin[ci])
    assert fallbacks <= 3
    assert sum(wins) / len(wins) < 34.0
    print(f"\nsc_halfsize: {differ} of {len(cases)} device results differ from the host's exact-division results")


def _digit16(n, k):
    nib = (n >> (4 * k)) & 15
    return nib - 16 * (nib >> 3) + ((n >> (4 * k - 1)) & 1 if k else 0)


def _digit256(n, k):
    b = (n >> (8 * k)) & 255
    return b - 256 * (b >> 7) + ((n >> (8 * k - 1)) & 1 if k else 0)


def _digits65536_pairs(n):
    d, carry = [], 0
    for k in range(16):
        x = ((n >> (16 * k)) & 0xffff) + carry
        carry = 1 if x >= 0x8000 else 0
        d.append(x - (carry << 16))
    return [(d[j] & 0xffff) | ((d[j + 8] & 0xffff) << 16) for j in range(8)]


@gpu
def test_window_words(dev):
    """cv_hs_scalars<true, false> (tri), <false, true> (throughput) and <false, false>: the 73 words against the
    digit16 / digit256 / digits65536_pairs definitions applied to the device's own (u, v, w, v_neg, nwin)."""
    cases = V.tri_digit_scalars(random.Random(2024))
    u, va, w, vneg, nwin, _ = _halfsize(dev, cases)
    inp = [words(h) + words(s) for h, s in cases]
    for form in (0, 1, 2):
        out = dev.run("cvd_hs_scalars", inp, 73, pre=(form,)).tolist()
        for ci in range(len(cases)):
            want = []
            for win in range(64):
                da = -_digit16(u[ci], win)
                dr = -_digit16(va[ci], win) if vneg[ci] else _digit16(va[ci], win)
                word = (da & 0x1f) | ((dr & 0x1f) << 5)
                if form == 0:
                    dlo, dhi = (_digit16(w[ci], win), _digit16(w[ci], 32 + win)) if win < 32 else (0, 0)
                    word |= ((dlo & 0x1f) << 10) | ((dhi & 0x1f) << 15)
                elif form == 2 and win % 2 == 0 and win < 32:
                    word |= ((_digit256(w[ci], win >> 1) & 0x1ff) << 10) | ((_digit256(w[ci], 16 + (win >> 1)) & 0x1ff) << 19)
                want.append(word)
            want += [nwin[ci]] + (_digits65536_pairs(w[ci]) if form == 1 else [0] * 8)
            assert out[ci] == want, (form, ci, [k for k in range(73) if out[ci][k] != want[k]][:4])


# ---------------------------------------------------------------- hashes
@gpu
def test_hashes(dev):
    """sha512_pre_msg (npre 32 and 64) and sha256_bytes (the alignbit / bitop3 device variants) against hashlib at
    the block-boundary lengths, aligned and unaligned message starts."""
    rng = random.Random(7)
    arena, recs, want = bytearray(16), [], []
    for ln in V.SHA_LENGTHS:
        pre = bytes(rng.randrange(256) for _ in range(64))
        m = bytes(rng.randrange(256) for _ in range(ln))
        for shift in (0,) + tuple(V.SHA_SHIFTS):
            arena += bytes((-len(arena)) % 8 + shift)
            off = len(arena)
            arena += m
            for npre in (32, 64):
                pw = np.frombuffer(pre[:npre] + bytes(64 - npre), np.uint32)
                recs.append([int(x) for x in pw] + [npre, off, ln])
                want.append((hashlib.sha512(pre[:npre] + m).digest(), hashlib.sha256(m).digest()))
    arena += bytes(16)
    buf = (ctypes.c_uint8 * len(arena)).from_buffer_copy(bytes(arena))
    out = dev.run("cvd_sha", recs, 24, post=(buf, ctypes.c_uint32(len(arena))))
    for rec, o, (d512, d256) in zip(recs, out, want):
        assert o[:16].tobytes() == d512, rec[16:]
        assert b"".join(int(x).to_bytes(4, "big") for x in o[16:]) == d256, rec[16:]


# ---------------------------------------------------------------- decode and tables
def _enc_int(e):
    return int.from_bytes(e, "little")


def _decode(e):
    try:
        return E.decode_point_0_1_0(e)
    except E.InvalidKeyError:
        return None


def _canonical(e):
    pt = _decode(e)
    return pt is not None and E.pt_encode(pt) == e


@pytest.fixture(scope="module")
def encodings(corpus):
    """(encoding, decoded point or None) for every distinct key and R of the golden corpus, the torsion matrix's 14 + 14,
    the max-limb encodings and 200 random strings."""
    m = np.load(os.path.join(GOLDEN, "ed25519_torsion_matrix.npz"))
    encs = {bytes(r) for r in corpus["pk"]} | {bytes(r[:32]) for r in corpus["sig"]}
    encs |= {bytes(r) for r in m["keys"]} | {bytes(r) for r in m["rs"]} | set(V.max_limb_cases()[0])
    rng = np.random.default_rng(77)
    encs |= {rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(200)}
    encs = sorted(encs)
    return encs, [_decode(e) for e in encs]


def _same_point(dev_xyz, ref):
    """Projective equality of the device's (X, Y, Z) with the reference point, Z != 0."""
    X, Y, Z = dev_xyz
    return Z % P != 0 and (X * ref[2] - ref[0] * Z) % P == 0 and (Y * ref[2] - ref[1] * Z) % P == 0


@gpu
def test_decode(dev, encodings):
    """ge_decode_0_1_0<false / true>, ge_decode2_0_1_0<false / true>, cv_r_canonical, ge_abyte_from_key."""
    encs, pts = encodings
    inp = np.array([words(_enc_int(e)) for e in encs], np.uint32)
    perm = np.random.default_rng(5).permutation(len(encs))
    inv = np.argsort(perm)                                   # encoding i is lane inv[i]'s second operand

    def check(what, e, pt, flag, enc, lim):
        assert int(flag) == (pt is not None), (what, e.hex())
        if pt is None:
            return
        y = _enc_int(e) & ((1 << 255) - 1)
        assert np.asarray(enc, np.uint32).tobytes() == E.pt_encode(pt), (what, e.hex())
        X, Y, Z, T = vals(lim)
        assert (X % P, Y, Z, T % P) == (pt[0], y, 1, pt[0] * y % P), (what, e.hex())     # y keeps its raw value
        assert_tight(lim, what)

    for lat in (0, 1):
        out = dev.run(f"cvd_decode_lat{lat}", inp, 58)
        out2 = dev.run(f"cvd_decode2_lat{lat}", np.hstack([inp, inp[perm]]), 98)
        for i, (e, pt) in enumerate(zip(encs, pts)):
            check(f"ge_decode_0_1_0<{lat}>", e, pt, out[i, 0], out[i, 1:9], out[i, 18:58])
            check(f"ge_decode2_0_1_0<{lat}>[0]", e, pt, out2[i, 0], out2[i, 1:9], out2[i, 9:49])
            check(f"ge_decode2_0_1_0<{lat}>[1]", e, pt, out2[inv[i], 49], out2[inv[i], 50:58], out2[inv[i], 58:98])
            y = _enc_int(e) & ((1 << 255) - 1)
            want_abyte = (y % P) | (0 if y % P in (1, P - 1) else (_enc_int(e) >> 255) << 255)
            assert from_words(out[i:i + 1, 10:18])[0] == want_abyte, e.hex()
            if pt is not None:
                assert int(out[i, 9]) == (E.pt_encode(pt) == e), e.hex()         # cv_r_canonical


def _multiples(pt, n=9):
    out, acc = [], E.IDENT
    for _ in range(n):
        out.append(acc)
        acc = E.pt_add(acc, pt)
    return out


def _check_table(tab, mult, entries, what):
    """Cached entries (Y+X, Y-X, Z, 2dT), 40 words each: entry k is projectively mult[k], Z != 0."""
    t = vals(tab)
    for k in entries:
        ypx, ymx, z, t2d = t[4 * k:4 * k + 4]
        X, Y, Z, T = mult[k]
        ok = z % P != 0 and (ypx * Z - (Y + X) * z) % P == 0 and (ymx * Z - (Y - X) * z) % P == 0 and \
            (t2d * Z - D2 * T * z) % P == 0
        assert ok, f"{what}: entry {k}"


@gpu
def test_tables(dev, encodings):
    """cv_hs_point_one<true / false> (one lane: half -1; split: halves 0 and 1) and cv_hs_points<false / true>: the
    flag, and entry k of the table is k * (-A) for a key, k * R for a canonical R, k * O otherwise."""
    encs, pts = encodings
    canon = [_canonical(e) for e in encs]
    neg_key = [_multiples(E.pt_neg(pt) if pt is not None else E.IDENT) for pt in pts]
    as_r = [_multiples(pt if c else E.IDENT) for pt, c in zip(pts, canon)]
    w = [words(_enc_int(e)) for e in encs]
    for lat in (1, 0):
        for is_r in (0, 1):
            for half, entries in ((-1, range(9)), (0, (0, 1, 3, 5, 7)), (1, (2, 4, 6, 8))):
                out = dev.run(f"cvd_point_one_lat{lat}", [x + [is_r, half + 1] for x in w], 364)
                for i, e in enumerate(encs):
                    assert int(out[i, 360]) == (canon[i] if is_r else pts[i] is not None), (lat, is_r, half, e.hex())
                    _check_table(out[i, :360], as_r[i] if is_r else neg_key[i], entries,
                                 f"point_one<{lat}> is_r={is_r} half={half} {e.hex()}")
        perm = np.random.default_rng(9 + lat).permutation(len(encs))
        out = dev.run(f"cvd_points_lat{lat}", [w[i] + w[j] for i, j in enumerate(perm)], 724)
        for i, j in enumerate(perm):
            assert int(out[i, 720]) == (pts[i] is not None) and int(out[i, 721]) == (pts[i] is not None and canon[j])
            _check_table(out[i, :360], neg_key[i], range(9), f"points<{lat}> tabA {encs[i].hex()}")
            _check_table(out[i, 360:720], as_r[j], range(9), f"points<{lat}> tabR {encs[j].hex()}")


# ---------------------------------------------------------------- quad: four lanes per point
def _scaled(pt, z):
    return tuple(c * z % P for c in pt)


def _pt_limbs(pt):
    return sum((to_limbs(c % P) for c in pt), [])


@pytest.fixture(scope="module")
def points():
    """Named points first, then about 100 random multiples of B, all with Z != 1 (scaled by a random element)."""
    rng = random.Random(31)
    tors = E.torsion_points()
    base = [("O", E.IDENT), ("B", E.BASE)] + [(f"T{k}", t) for k, t in enumerate(tors)]
    base += [("-B", E.pt_neg(E.BASE)), ("B+T1", E.pt_add(E.BASE, tors[1])), ("-(B+T1)", E.pt_neg(E.pt_add(E.BASE, tors[1])))]
    base += [(f"[r{k}]B", E.pt_mul(rng.randrange(L), E.BASE)) for k in range(100)]
    return [(name, _scaled(pt, rng.randrange(1, P))) for name, pt in base]


def _check_points(out, refs, names, what):
    """After a step the four lanes' (X, Y, Z, T): X/Z, Y/Z equal the reference, T Z == X Y, and the limbs are tight."""
    assert_tight(out, what)
    v = vals(out)
    for i, (ref, name) in enumerate(zip(refs, names)):
        X, Y, Z, T = v[4 * i:4 * i + 4]
        assert _same_point((X, Y, Z), ref), f"{what}: wrong point at {name}"
        assert (T * Z - X * Y) % P == 0, f"{what}: T Z != X Y at {name}"


@gpu
@pytest.mark.parametrize("seq", [1, 0], ids=["seq", "ilp"])
def test_quad_dbl_and_to_cached(dev, points, seq):
    """quad_dbl on every point (the identity, B, each torsion point, -P, random multiples), then again on its own
    output (limbs as a previous step leaves them); quad_to_cached of both."""
    names, pts = [n for n, _ in points], [p for _, p in points]
    inp = np.array([_pt_limbs(p) for p in pts], np.uint32)
    refs = pts
    for rnd in range(3):
        c = dev.quad("cvd_quad_to_cached", seq, inp, 40)
        assert_tight(c, "quad_to_cached")
        for i, (X, Y, Z, T) in enumerate(refs):
            assert_vals(c[i], [Y + X, Y - X, Z, D2 * T], f"quad_to_cached round {rnd} {names[i]}") if rnd == 0 else None
            _check_table(c[i], [refs[i]], [0], f"quad_to_cached round {rnd} {names[i]}")
        inp = dev.quad("cvd_quad_dbl", seq, inp, 40)
        refs = [E.pt_dbl(p) for p in refs]
        _check_points(inp, refs, [f"2^{rnd + 1} {n}" for n in names], "quad_dbl")


def _add_cases(points, rng):
    """(name, P, Q, digit) for the cached-table operand forms: every digit -8 .. 8 over random pairs, plus the named
    cases P + (-P), P + P, P + O, O + O, torsion operands on both sides."""
    by = dict(points)
    rnd = [p for n, p in points if n.startswith("[r")]
    cases = [(f"d={d}", rng.choice(rnd), rng.choice(rnd), d) for d in range(-8, 9) for _ in range(3)]
    Pt, O = by["[r0]B"], by["O"]
    cases += [("P + (-P)", Pt, Pt, -1), ("P + P", Pt, Pt, 1), ("P + O (digit 0)", Pt, by["[r1]B"], 0),
              ("P + O (table of O)", Pt, O, 1), ("O + O (digit 0)", O, Pt, 0), ("O + O (table of O)", O, O, 3),
              ("O + P", O, Pt, 1), ("O + digit -8", O, Pt, -8), ("P + digit -8", Pt, by["B"], -8)]
    for k in range(8):
        cases += [(f"T{k} + T{(3 * k + 1) % 8}", by[f"T{k}"], by[f"T{(3 * k + 1) % 8}"], 1),
                  (f"P + [-8]T{k}", Pt, by[f"T{k}"], -8), (f"T{k} + (-T{k})", by[f"T{k}"], by[f"T{k}"], -1)]
    return cases


def _smul(d, pt):
    r = E.pt_mul(abs(d), pt)
    return E.pt_neg(r) if d < 0 else r


@gpu
@pytest.mark.parametrize("seq", [1, 0], ids=["seq", "ilp"])
def test_quad_add_cached_tables(dev, points, seq):
    """quad_add with its operand from quad_cached_coord and from quad_any_coord's cached format, over a
    ge_cached_multiples8 table built in the same kernel; the results fed once more through quad_add."""
    cases = _add_cases(points, random.Random(41))
    names = [c[0] for c in cases]
    for mode in (0, 2):
        inp = np.array([_pt_limbs(p) + _pt_limbs(q) + [d & 0xffffffff] + [0] * 7 for _, p, q, d in cases], np.uint32)
        refs = [p for _, p, _, _ in cases]
        for rnd in range(2):
            out = dev.quad("cvd_quad_add", seq, inp, 40, pre=(mode,), post=(None, ctypes.c_uint32(0)))
            refs = [E.pt_add(r, _smul(d, q)) for r, (_, _, q, d) in zip(refs, cases)]
            _check_points(out, refs, names, f"quad_add mode {mode} round {rnd}")
            inp[:, :40] = out


ROW = 129 * 32          # CV_BTAB_ENTRIES * CV_BTAB_STRIDE: one CV_BCOMB row, k * 2^(64 j) * B for k = 0 .. 128


def _affine_rows(pt, entries):
    """k * pt (k = 0 .. entries - 1) as affine rows (y+x, y-x, 2dxy | pad to 32 words), row 0 the identity."""
    rows, acc = [], E.IDENT
    for _ in range(entries):
        x, y = E.pt_affine(acc)
        rows.append(to_limbs((y + x) % P) + to_limbs((y - x) % P) + to_limbs(D2 * x * y % P) + [0, 0])
        acc = E.pt_add(acc, pt)
    return np.array(rows, np.uint32)


@gpu
@pytest.mark.parametrize("seq", [1, 0], ids=["seq", "ilp"])
def test_quad_add_affine_rows(dev, points, seq):
    """quad_add with its operand from quad_precomp_coord (CV_BCOMB rows and a keyed row; digits 0, negative, +-128;
    ident_row both ways) and from quad_any_coord's affine format (CV_BCOMB rows 0 and 2, the tri form's)."""
    rng = random.Random(43)
    by = dict(points)
    rnd = [p for n, p in points if n.startswith("[r")]
    A = E.pt_add(E.pt_mul(rng.randrange(L), E.BASE), E.torsion_points()[3])            # a mixed-order key point
    keyed = _affine_rows(A, 130).reshape(-1)
    bj = [E.pt_mul(1 << (64 * j), E.BASE) for j in range(4)]
    digits = [0, 1, -1, 2, -8, 8, 127, -127, 128, -128]
    # (name, P, table point, digit, word offset, from aux, ident_row)
    cases = []
    for j in range(4):
        for d in digits + [rng.randrange(-128, 129) for _ in range(4)]:
            cases.append((f"CV_BCOMB row {j} d={d}", rng.choice(rnd), bj[j], d, j * ROW, 0, 1))
    for j in range(3):          # entry k - 1 holds k P: the same rows entered one entry up
        for d in digits:
            cases.append((f"CV_BCOMB row {j} d={d} no identity row", rng.choice(rnd), bj[j], d, j * ROW + 32, 0, 0))
    for d in digits + [rng.randrange(-128, 129) for _ in range(6)]:
        cases.append((f"keyed row d={d}", rng.choice(rnd), A, d, 0, 1, 1))
        cases.append((f"keyed row d={d} no identity row", rng.choice(rnd), A, d, 32, 1, 0))
    cases += [("O + digit 0", by["O"], bj[0], 0, 0, 0, 1), ("O + digit -8", by["O"], bj[0], -8, 0, 0, 1),
              ("P + (-P)", _scaled(E.pt_mul(5, A), 7), A, -5, 0, 1, 1), ("P + P", _scaled(E.pt_mul(5, A), 9), A, 5, 0, 1, 1)]
    for mode in (1, 3):
        sel = [c for c in cases if mode == 1 or (not c[5] and c[6])]
        inp = np.array([_pt_limbs(p) + [0] * 40 + [d & 0xffffffff, off, aux, 32, ident, 0, 0, 0]
                        for _, p, _, d, off, aux, ident in sel], np.uint32)
        buf = keyed.ctypes.data_as(ctypes.c_void_p)
        out = dev.quad("cvd_quad_add", seq, inp, 40, pre=(mode,), post=(buf, ctypes.c_uint32(keyed.size)))
        refs = [E.pt_add(p, _smul(d, q)) for _, p, q, d, _, _, _ in sel]
        _check_points(out, refs, [c[0] for c in sel], f"quad_add mode {mode}")


@gpu
@pytest.mark.parametrize("seq", [1, 0], ids=["seq", "ilp"])
def test_tri_rotation_sum(dev, points, seq):
    """The tail of cv_tri_hs_straus (row_ror:4, row_ror:8): four points, one per quad of a 16-lane group; every quad
    ends with the sum of the four."""
    rng = random.Random(47)
    pts = [p for _, p in points]
    groups = [[pts[0]] * 4, [pts[0], pts[1], pts[0], E.pt_neg(pts[1])], pts[2:6], pts[6:10]]
    groups += [[rng.choice(pts) for _ in range(4)] for _ in range(28)]
    inp = np.array([_pt_limbs(p) for g in groups for p in g], np.uint32)
    out = dev.quad("cvd_tri_sum", seq, inp, 40)
    refs, names = [], []
    for gi, g in enumerate(groups):
        s = E.IDENT
        for p in g:
            s = E.pt_add(s, p)
        refs += [s] * 4
        names += [f"group {gi} quad {c}" for c in range(4)]
    _check_points(out, refs, names, "tri rotation sum")


@gpu
@pytest.mark.parametrize("seq", [1, 0], ids=["seq", "ilp"])
def test_quad_chain(dev, points, seq):
    """Eight windows of four quad_dbl and one quad_add, the point checked after every one of the 40 steps."""
    rng = random.Random(53)
    by = dict(points)
    rnd = [p for n, p in points if n.startswith("[r")]
    cases = [(by["O"], rnd[0], [0, 0, 1, -8, 8, 0, -1, 3]), (by["T1"], by["T3"], [1, -1, 8, -8, 0, 5, -5, 7]),
             (rnd[1], rnd[1], [-1, 1, -2, 2, -4, 4, -8, 8])]
    cases += [(rng.choice(rnd), rng.choice(rnd), [rng.randrange(-8, 9) for _ in range(8)]) for _ in range(13)]
    inp = np.array([_pt_limbs(p) + _pt_limbs(q) + [d & 0xffffffff for d in ds] for p, q, ds in cases], np.uint32)
    out = dev.quad("cvd_quad_chain", seq, inp, 1600)
    for ci, (p, q, ds) in enumerate(cases):
        refs, acc = [], p
        for d in ds:
            for _ in range(4):
                acc = E.pt_dbl(acc)
                refs.append(acc)
            acc = E.pt_add(acc, _smul(d, q))
            refs.append(acc)
        _check_points(out[ci].reshape(40, 40), refs, [f"case {ci} step {k}" for k in range(40)], "quad chain")


# ---------------------------------------------------------------- verdict bit packing
@gpu
def test_ballot_packing(dev):
    """cv_quad_ballot_bits (lanes 0, 4, .., 60 -> 16 bits) and the tri kernel's packing (lanes 0, 16, 32, 48 -> 4 bits)
    over 1,000 random masks, 0, all ones and every single bit."""
    rng = random.Random(59)
    masks = [0, 2**64 - 1] + [1 << k for k in range(64)] + [rng.getrandbits(64) for _ in range(1000)]
    out = dev.run("cvd_ballot", [words(m, 2) for m in masks], 2).tolist()
    for m, (q, t) in zip(masks, out):
        assert q == sum(((m >> (4 * j)) & 1) << j for j in range(16)), hex(m)
        assert t == sum(((m >> (16 * j)) & 1) << j for j in range(4)), hex(m)
