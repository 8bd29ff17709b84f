"""cv_notarise_batch's outputs under the header's Conventions (include/cordaverify.h): every output carved by
tests/guarded.py at the alignment of its C type and no more, poisoned and guard-banded.  A successful call writes every
byte of every output it is given and nothing around it, whatever they held; optional outputs may be NULL; records and
signatures are zero where the contract says zero.  Two poison bytes, so a result ORed into what was there shows.
"""
import ctypes

import numpy as np
import pytest

import notarise_batches as B
import notarise_cases as C
from corda_amd import native
from guarded import Guarded

pytestmark = pytest.mark.gpu

NTX = 65
OPTIONAL = ("ids", "first_bad", "req_missing")


@pytest.fixture(scope="module")
def signer(engine):
    s = native.Signer(engine, B.NOTARY_SEED)
    yield s
    s.close()


@pytest.fixture(scope="module")
def batch(engine, corpus, signer):
    b = B.make_batch(engine, corpus, NTX)
    want, ref = B.compose(engine, signer, b)
    ref.close()
    return b, want


def carve(b, fill):
    ns, nreq = int(b["tx_input_count"].sum()), int(b["reqs"][6].size - 1)
    spec = [("outcome", NTX, 1), ("ids", 32 * NTX, 1), ("notary_sig", 64 * NTX, 1), ("first_bad", 4 * NTX, 4),
            ("req_missing", nreq, 1), ("state_conflict", ns, 1), ("consumed_id", 32 * ns, 1), ("consumed_index", 4 * ns, 4),
            ("consumed_caller", 4 * ns, 4)]
    return Guarded(spec, fill), spec


def as_array(g, name, nbytes):
    """The output inside the guarded allocation as the array Engine.notarise_batch passes on (no copy)."""
    off = g.slots[name][0]
    return g.buf[off:off + nbytes]


@pytest.mark.parametrize("fill", (0x00, 0xFF, 0xA5))
@pytest.mark.parametrize("nulls", (False, True))
def test_outputs_written_whole_and_nothing_around(engine, signer, batch, fill, nulls):
    b, want = batch
    g, spec = carve(b, fill)
    out = {name: None if nulls and name in OPTIONAL else as_array(g, name, nbytes) for name, nbytes, _ in spec}
    uniq = B.open_set(engine, b)
    # the binding hands the arrays on by address: the odd and 4-mod-8 addresses reach the library as they are
    for name, a in out.items():
        assert a is None or native._p(a) == g.ptr(name)
    B.call(engine, uniq, signer, b, out=out)
    uniq.close()
    g.check_guards(f"fill {fill:#x} nulls {nulls}")
    dt = dict(first_bad=np.uint32, consumed_index=np.uint32, consumed_caller=np.uint32)
    for name, nbytes, _ in spec:
        if out[name] is None:
            assert g.untouched(name)
            continue
        got = g.read(name, dt.get(name, np.uint8))
        assert np.array_equal(got, want[name].reshape(-1)), (name, fill)
    outcome = g.read("outcome")
    sig = g.read("notary_sig", shape=(NTX, 64))
    assert not sig[outcome != C.SUCCESS].any() and sig[outcome == C.SUCCESS].any(1).all()
    sc = g.read("state_conflict")
    assert set(sc.tolist()) <= {0, 1}
    assert not g.read("consumed_id", shape=(-1, 32))[sc == 0].any()
    assert not g.read("consumed_index", np.uint32)[sc == 0].any() and not g.read("consumed_caller", np.uint32)[sc == 0].any()
    per_tx = np.repeat(outcome, b["tx_input_count"])
    assert not sc[per_tx != C.CONFLICT].any()            # records only for the states of a conflicting transaction
