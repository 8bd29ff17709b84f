#!/usr/bin/env python3
"""Writes tests/golden/ed25519_torsion_matrix.npz: small-order R against small-order keys.

The golden corpus (make_golden.py) has torsion and mixed-order keys and R + T8, but no small-order R and no
R with x = 0 and the sign bit set.  That is the class where the half-size equation [v]R + [u]A + [w]B == O
differs from the reference's byte compare unless v is odd and R's encoding is checked for canonicity
(cv_r_canonical, in particular its y == p - 1 branch).  The matrix:

  14 keys : the 8 torsion points, enc_y(1, 1), enc_y(p-1, 1), enc_y(p, 0), enc_y(p, 1), enc_y(p+1, 0),
            enc_y(p+1, 1)                                  (enc_y(y, s) = y | s << 255, 32 bytes LE)
  14 R    : the 8 canonical torsion encodings; y + p where that fits below 2^255 (enc_y(p+1, 0), enc_y(p, 0),
            enc_y(p, 1)); the sign bit set for y = 1 and y = p - 1; enc_y(p+1, 1)
  S       : 0, L, 2L
  6 random 32-byte messages per cell (fixed seed)

Expected values are ed25519_ref.verify_ex's.  Arrays as in ed25519_corpus.npz (pk, sig, arena, off, len,
verdict, status) plus key_id, r_id, s_id per row, the encodings (keys, rs, svals) and key_never / r_never:
the encodings that can never be accepted BY RULE (a key the oracle refuses; an R whose bytes are not the
encoding of the point they decode to — non-canonical y, or x = 0 with the sign bit set).

    python tests/golden/make_torsion_matrix.py
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import ed25519_ref as E  # noqa: E402

P, L = E.P, E.L
SEED = 20261019
MSGS_PER_CELL = 6


def enc_y(y: int, sign: int) -> bytes:
    assert 0 <= y < 1 << 255
    return (y | (sign << 255)).to_bytes(32, "little")


def key_encodings():
    return [E.pt_encode(t) for t in E.torsion_points()] + [
        enc_y(1, 1), enc_y(P - 1, 1), enc_y(P, 0), enc_y(P, 1), enc_y(P + 1, 0), enc_y(P + 1, 1)]


def r_encodings():
    tors = [E.pt_encode(t) for t in E.torsion_points()]
    plus_p = []
    for e in tors:
        v = int.from_bytes(e, "little")
        y, sign = v & ((1 << 255) - 1), v >> 255
        if y + P < 1 << 255:
            plus_p.append(enc_y(y + P, sign))
    assert sorted(plus_p) == sorted([enc_y(P + 1, 0), enc_y(P, 0), enc_y(P, 1)])
    return tors + plus_p + [enc_y(1, 1), enc_y(P - 1, 1), enc_y(P + 1, 1)]


def never_key(e: bytes) -> bool:
    try:
        E.decode_point_0_1_0(e)
        return False
    except E.InvalidKeyError:
        return True


def never_r(e: bytes) -> bool:
    try:
        return E.pt_encode(E.decode_point_0_1_0(e)) != e
    except E.InvalidKeyError:
        return True


def build():
    keys, rs, svals = key_encodings(), r_encodings(), [0, L, 2 * L]
    assert len(keys) == 14 and len(set(keys)) == 14 and len(rs) == 14 and len(set(rs)) == 14
    rng = random.Random(SEED)
    rows = []
    for ki, k in enumerate(keys):
        for ri, r in enumerate(rs):
            for si, s in enumerate(svals):
                for _ in range(MSGS_PER_CELL):
                    rows.append((ki, ri, si, rng.randbytes(32)))
    n = len(rows)
    pk = np.zeros((n, 32), np.uint8)
    sig = np.zeros((n, 64), np.uint8)
    arena = np.zeros(32 * n, np.uint8)
    off = np.arange(n, dtype=np.uint64) * 32
    ln = np.full(n, 32, np.uint32)
    verdict = np.zeros(n, np.uint8)
    status = np.zeros(n, np.uint8)
    for i, (ki, ri, si, m) in enumerate(rows):
        s = rs[ri] + svals[si].to_bytes(32, "little")
        pk[i] = np.frombuffer(keys[ki], np.uint8)
        sig[i] = np.frombuffer(s, np.uint8)
        arena[32 * i:32 * i + 32] = np.frombuffer(m, np.uint8)
        st, ok = E.verify_ex(keys[ki], m, s)
        status[i] = 0 if st == E.ST_OK else 1
        verdict[i] = 1 if (st == E.ST_OK and ok) else 0
    out = dict(pk=pk, sig=sig, arena=arena, off=off, len=ln, verdict=verdict, status=status,
               key_id=np.array([r[0] for r in rows], np.uint8), r_id=np.array([r[1] for r in rows], np.uint8),
               s_id=np.array([r[2] for r in rows], np.uint8),
               keys=np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32),
               rs=np.frombuffer(b"".join(rs), np.uint8).reshape(-1, 32),
               svals=np.frombuffer(b"".join(s.to_bytes(32, "little") for s in svals), np.uint8).reshape(-1, 32),
               key_never=np.array([never_key(k) for k in keys], np.uint8),
               r_never=np.array([never_r(r) for r in rs], np.uint8))
    return out


def check(m):
    """The conditions tests/test_torsion_matrix.py asserts on the committed file."""
    acc = m["verdict"] == 1
    assert acc.sum() >= 150 and (~acc).sum() >= 2000, (int(acc.sum()), int((~acc).sum()))
    for ids, never in ((m["key_id"], m["key_never"]), (m["r_id"], m["r_never"])):
        for k in range(14):
            assert bool(never[k]) != bool(acc[ids == k].any()), k
    assert np.array_equal(m["status"] == 1, m["key_never"][m["key_id"]] == 1)


if __name__ == "__main__":
    m = build()
    check(m)
    path = os.path.join(HERE, "ed25519_torsion_matrix.npz")
    np.savez_compressed(path, **m)
    print(f"{path}: {len(m['pk'])} rows, {int(m['verdict'].sum())} accepted, {os.path.getsize(path)} bytes")
