"""Small-order R against small-order keys (tests/golden/ed25519_torsion_matrix.npz, written by
tests/golden/make_torsion_matrix.py from the Python oracle): the class where the half-size equation
[v]R + [u]A + [w]B == O differs from the reference's byte compare unless v is odd and R's encoding is canonical
(cv_r_canonical and its y == p - 1 branch).  No GPU: the fixture's own conditions, the C oracle, and the per-lane
code on the host harness in its five forms."""
import ctypes
import os

import numpy as np
import pytest

import ed25519_ref as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FORMS = ["full", "hs", "fused0", "fused1", "keyed"]


@pytest.fixture(scope="module")
def matrix():
    return dict(np.load(os.path.join(GOLDEN, "ed25519_torsion_matrix.npz")))


def _b(x: bytes):
    return (ctypes.c_uint8 * max(1, len(x))).from_buffer_copy(x + b"\0")


def test_fixture_conditions(matrix):
    m = matrix
    n = len(m["pk"])
    assert n == 14 * 14 * 3 * 6
    acc = m["verdict"] == 1
    assert acc.sum() >= 150 and (~acc).sum() >= 2000
    # every encoding is accepted somewhere or can never be: a key the oracle refuses; an R that is not the encoding
    # of the point it decodes to (non-canonical y, or x = 0 with the sign bit set)
    p = E.P
    for k in range(14):
        key, r = bytes(m["keys"][k]), bytes(m["rs"][k])
        try:
            E.decode_point_0_1_0(key)
            key_never = False
        except E.InvalidKeyError:
            key_never = True
        r_int = int.from_bytes(r, "little")
        y, sign = r_int & ((1 << 255) - 1), r_int >> 255
        r_never = y >= p or (sign == 1 and y % p in (1, p - 1))
        assert r_never == (E.pt_encode(E.decode_point_0_1_0(r)) != r)
        assert bool(m["key_never"][k]) == key_never and bool(m["r_never"][k]) == r_never
        assert bool(acc[m["key_id"] == k].any()) != key_never, f"key {k}"
        assert bool(acc[m["r_id"] == k].any()) != r_never, f"R {k}"
    assert m["r_never"].sum() >= 6          # y + p (3), sign bit on y = +-1 (2), both (1)
    assert np.array_equal(m["status"] == 1, m["key_never"][m["key_id"]] == 1)
    assert not (acc & (m["status"] == 1)).any()
    # the rows are what the ids say
    svals = [0, E.L, 2 * E.L]
    for i in range(0, n, 7):
        assert bytes(m["pk"][i]) == bytes(m["keys"][m["key_id"][i]])
        assert bytes(m["sig"][i][:32]) == bytes(m["rs"][m["r_id"][i]])
        assert int.from_bytes(bytes(m["sig"][i][32:]), "little") == svals[m["s_id"][i]]
    assert int(m["len"].min()) == 32 and int(m["off"][-1]) + 32 == m["arena"].size
    assert os.path.getsize(os.path.join(GOLDEN, "ed25519_torsion_matrix.npz")) < 1 << 20


def test_fixture_sample_against_python_oracle(matrix):
    """Every 9th row (and every accepted one) recomputed by ed25519_ref.verify_ex: the file is this project's oracle's."""
    m = matrix
    rows = sorted(set(range(0, len(m["pk"]), 9)) | set(np.nonzero(m["verdict"])[0].tolist()))
    for i in rows:
        msg = m["arena"][int(m["off"][i]):int(m["off"][i]) + int(m["len"][i])].tobytes()
        st, ok = E.verify_ex(bytes(m["pk"][i]), msg, bytes(m["sig"][i]))
        assert (1 if (st == 0 and ok) else 0, 0 if st == 0 else 1) == (m["verdict"][i], m["status"][i]), i


def test_matrix_against_c_oracle(matrix, oracle_c):
    m = matrix
    ref, rst = oracle_c.verify_batch(m["pk"], m["sig"], m["arena"], m["off"], m["len"], nthreads=8)
    bad = np.nonzero((ref != m["verdict"]) | (rst != m["status"]))[0]
    assert bad.size == 0, [(int(m["key_id"][i]), int(m["r_id"][i]), int(m["s_id"][i])) for i in bad[:8]]


def test_r_canonical_on_host_harness(host_harness, matrix, corpus):
    """cv_r_canonical equals "the bytes are the encoding of the point they decode to" on the matrix's 14 + 14 encodings
    (y = p - 1 and y = 1 with the sign bit set, y + p) and on every decodable key and R of the golden corpus."""
    encs = {bytes(r) for r in matrix["keys"]} | {bytes(r) for r in matrix["rs"]}
    encs |= {bytes(r) for r in corpus["pk"]} | {bytes(r[:32]) for r in corpus["sig"]}
    seen = set()
    for e in sorted(encs):
        try:
            want = E.pt_encode(E.decode_point_0_1_0(e)) == e
        except E.InvalidKeyError:
            continue
        assert host_harness.cvh_r_canonical(e) == int(want), e.hex()
        seen.add(want)
    assert seen == {True, False}


@pytest.mark.parametrize("form", FORMS)
def test_matrix_on_host_harness(host_harness, matrix, form):
    """cvh_verify, cvh_verify_hs, cvh_verify_hs_fused (lat 0 and 1) and cvh_verify_keyed: verdict and key status of
    every row equal the oracle's."""
    H, m = host_harness, matrix
    sc = (ctypes.c_uint32 * 73)()
    bad = []
    for i in range(len(m["pk"])):
        pk, sig = _b(m["pk"][i].tobytes()), _b(m["sig"][i].tobytes())
        msg = m["arena"][int(m["off"][i]):int(m["off"][i]) + int(m["len"][i])].tobytes()
        st = ctypes.c_int(0)
        if form == "full":
            v = H.cvh_verify(pk, sig, _b(msg), len(msg), ctypes.byref(st))
        elif form == "hs":
            v = H.cvh_verify_hs(pk, sig, _b(msg), len(msg), ctypes.byref(st), sc)
        elif form.startswith("fused"):
            v = H.cvh_verify_hs_fused(pk, sig, _b(msg), len(msg), ctypes.byref(st), int(form[-1]))
        else:
            v = H.cvh_verify_keyed(pk, sig, _b(msg), len(msg), ctypes.byref(st))
        if (v, st.value) != (m["verdict"][i], m["status"][i]):
            bad.append((int(m["key_id"][i]), int(m["r_id"][i]), int(m["s_id"][i]), v, st.value))
    assert not bad, (len(bad), bad[:8])
