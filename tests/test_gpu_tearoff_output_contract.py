"""The outputs of cv_filtered_verify and cv_tearoff_sign_batch under the header's Conventions (include/cordaverify.h):
every output carved by tests/guarded.py at the alignment of its C type and no more, poisoned and guard-banded.  A
successful call writes every byte of every output it is given and nothing around it, whatever they held; optional
outputs may be NULL; the signature of a refused tear-off is 64 zero bytes whatever the buffer held before.  Three poison
bytes, so a result ORed into what was there shows.
"""
import numpy as np
import pytest

import tearoff_cases as C
from corda_amd import native
from guarded import Guarded

pytestmark = pytest.mark.gpu

NTX = 65
SEED = bytes(range(32))


@pytest.fixture(scope="module")
def signer(engine):
    s = native.Signer(engine, SEED)
    yield s
    s.close()


@pytest.fixture(scope="module")
def batch(engine, signer):
    """The batch and what the calls return into fresh arrays."""
    f = C.flatten(C.service_batch(NTX, seed=31))
    args = (f["arena"], f["leaf_off"], f["leaf_len"], f["txb"], f["kind"], f["left"], f["right"], f["node_hash"],
            f["tree_begin"], f["root"])
    want = dict(zip(("outcome", "first_bad", "sig_out"), engine.tearoff_sign_batch(signer, *args, f["leaf_pre"])))
    want.update(zip(("verdict", "status"), engine.filtered_verify(*args)))
    assert set(want["outcome"].tolist()) == set(range(7)) and set(want["status"].tolist()) == {0, 2, 4}
    return f, args, want


def as_array(g, name, nbytes):
    """The output inside the guarded allocation as the array the binding passes on (no copy)."""
    off = g.slots[name][0]
    return g.buf[off:off + nbytes]


@pytest.mark.parametrize("fill", (0x00, 0xFF, 0xA5))
@pytest.mark.parametrize("nulls", (False, True))
def test_sign_batch_outputs_written_whole_and_nothing_around(engine, signer, batch, fill, nulls):
    f, args, want = batch
    spec = [("outcome", NTX, 1), ("first_bad", 4 * NTX, 4), ("sig_out", 64 * NTX, 1)]
    g = Guarded(spec, fill)
    out = [None if nulls and name == "first_bad" else as_array(g, name, nbytes) for name, nbytes, _ in spec]
    for (name, _, _), a in zip(spec, out):
        assert a is None or native._p(a) == g.ptr(name)      # the odd and 4-mod-8 addresses reach the library as they are
    lib, P = native.load(), native._p
    nodes = [P(f[k]) for k in ("kind", "left", "right", "node_hash")]
    rc = lib.cv_tearoff_sign_batch(engine._h, signer._h, NTX, P(f["arena"]), f["arena_bytes"], P(f["leaf_off"]),
                                   P(f["leaf_len"]), P(f["txb"]), len(f["kind"]), *nodes, P(f["tree_begin"]), P(f["root"]),
                                   P(f["leaf_pre"]), *[P(a) for a in out])
    assert rc == 0
    g.check_guards(f"fill {fill:#x} nulls {nulls}")
    outcome = g.read("outcome")
    assert np.array_equal(outcome, want["outcome"])
    if nulls:
        assert g.untouched("first_bad")
    else:
        assert np.array_equal(g.read("first_bad", np.uint32), want["first_bad"])
    sig = g.read("sig_out", shape=(NTX, 64))
    assert np.array_equal(sig, want["sig_out"])
    assert not sig[outcome != C.SUCCESS].any() and sig[outcome == C.SUCCESS].any(1).all()


@pytest.mark.parametrize("fill", (0x00, 0xFF, 0xA5))
@pytest.mark.parametrize("nulls", (False, True))
def test_filtered_verify_outputs_written_whole_and_nothing_around(engine, batch, fill, nulls):
    f, args, want = batch
    spec = [("verdict", NTX, 1), ("status", NTX, 1)]
    g = Guarded(spec, fill)
    lib, P = native.load(), native._p
    nodes = [P(f[k]) for k in ("kind", "left", "right", "node_hash")]
    rc = lib.cv_filtered_verify(engine._h, NTX, P(f["arena"]), f["arena_bytes"], P(f["leaf_off"]), P(f["leaf_len"]),
                                P(f["txb"]), len(f["kind"]), *nodes, P(f["tree_begin"]), P(f["root"]),
                                g.ptr("verdict"), None if nulls else g.ptr("status"))
    assert rc == 0
    g.check_guards(f"fill {fill:#x} nulls {nulls}")
    assert np.array_equal(g.read("verdict"), want["verdict"])
    if nulls:
        assert g.untouched("status")
    else:
        assert np.array_equal(g.read("status"), want["status"])
