"""Two input classes through every GPU kernel form, verdicts and key status bytes exact:
  - the torsion matrix (tests/golden/ed25519_torsion_matrix.npz: small-order R against small-order keys, where the
    half-size equation needs v odd and the canonical-R check to agree with the reference's byte compare);
  - the max-limb encodings of test_device_logic.py::test_limb_bounds_on_max_limb_encodings (y in [2^255 - 64, 2^255),
    y = 2^255 - 2^j, S at 2^256 - 1, 2^255 and around L), which until now only the host harness saw.
Forms: shuffled and tiled, default options, (quad_max, tri_max) forced to the throughput / quad / tri kernels, the
keyed path, and n = 4,096 and 9,001 sampled with replacement (the default latency forms)."""
import os

import numpy as np
import pytest

import device_vectors as V
import ed25519_ref as E
from test_gpu_parity import _bits, _dedupe, _opts

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def matrix():
    return dict(np.load(os.path.join(GOLDEN, "ed25519_torsion_matrix.npz")))


@pytest.fixture(scope="module")
def maxlimb(oracle_c):
    """The 184 max-limb cases tiled to 1,000 records; expected values from the C oracle, which must agree with the
    Python oracle on the 184."""
    _, cases = V.max_limb_cases()
    assert len(cases) == 184
    n = len(cases)
    pk = np.frombuffer(b"".join(c[0] for c in cases), np.uint8).reshape(n, 32).copy()
    sig = np.frombuffer(b"".join(c[1] for c in cases), np.uint8).reshape(n, 64).copy()
    ln = np.array([len(c[2]) for c in cases], np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1])
    arena = np.frombuffer(b"".join(c[2] for c in cases) + bytes(16), np.uint8).copy()
    ref, rst = oracle_c.verify_batch(pk, sig, arena, off, ln, nthreads=8)
    for i, (p, s, m) in enumerate(cases):
        st, ok = E.verify_ex(p, m, s)
        assert (int(ref[i]), int(rst[i])) == (1 if (st == 0 and ok) else 0, 0 if st == 0 else 1), i
    sel = np.arange(1000) % n
    return dict(pk=pk[sel], sig=sig[sel], arena=arena, off=off[sel], len=ln[sel], verdict=ref[sel].astype(np.uint8),
                status=rst[sel].astype(np.uint8))


@pytest.fixture(params=["torsion", "maxlimb"])
def data(request, matrix, maxlimb):
    return matrix if request.param == "torsion" else maxlimb


def _check(engine, d, sel=None, keyed=False):
    sel = np.arange(len(d["pk"])) if sel is None else sel
    pk, sig, off, ln = d["pk"][sel], d["sig"][sel], d["off"][sel], d["len"][sel]
    if keyed:
        keys, kidx = _dedupe(pk)
        bitmap, status = engine.verify_batch_keyed(keys, kidx, sig, d["arena"], off, ln)
    else:
        bitmap, status = engine.verify_batch(pk, sig, d["arena"], off, ln)
    bad = np.nonzero(_bits(bitmap, sel.size) != d["verdict"][sel].astype(bool))[0]
    assert bad.size == 0, (bad.size, [(bytes(pk[i]).hex(), bytes(sig[i]).hex()) for i in bad[:4]])
    assert np.array_equal(status, d["status"][sel])


def test_default_options(engine, data):
    _check(engine, data)


def test_shuffled_and_tiled(engine, data):
    """A shuffled order, tiled 3x: verdicts follow the records (no cross-lane leaks)."""
    rng = np.random.default_rng(1)
    _check(engine, data, np.concatenate([rng.permutation(len(data["pk"])) for _ in range(3)]))


@pytest.mark.parametrize("quad_max,tri_max", [(0, 0), (1 << 22, 0), (1 << 22, 1 << 20)])
def test_forced_forms(engine, data, quad_max, tri_max):
    """(0, 0) the throughput kernels, (2^22, 0) the quad form, (2^22, 2^20) the tri-chain form."""
    with _opts(engine, quad_max=quad_max, tri_max=tri_max):
        _check(engine, data)
        _check(engine, data, keyed=True)


def test_keyed_path(engine, data):
    _check(engine, data, keyed=True)


@pytest.mark.parametrize("n", [4096, 9001])
def test_default_latency_sizes(engine, data, n):
    rng = np.random.default_rng(n + 11)
    _check(engine, data, rng.integers(0, len(data["pk"]), n))
