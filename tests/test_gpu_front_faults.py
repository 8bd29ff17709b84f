"""The argument checks of the calls that take leaves, signatures and CompositeKey requirements as flat arrays, with a
live engine: a valid batch of two transactions passes, and the same batch with each single fault
of tests/front_faults.py's table returns the code recorded there — before any device work, so every output, carved by
tests/guarded.py and poisoned, and every guard band around it stays as it was.
"""
import pytest

import front_faults as F
import notarise_batches as B
from corda_amd import native
from guarded import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture
def handles(engine):
    """A signer and an empty uniqueness set of its own for every family: the valid notarise batch commits a state."""
    signer = native.Signer(engine, B.NOTARY_SEED)
    uniq = native.UniquenessSet(engine, 64)
    yield {"ctx": engine._h, "uniq": uniq._open(), "signer": signer._h}
    uniq.close()
    signer.close()


@pytest.mark.parametrize("family", sorted(F.FAMILIES))
def test_valid_batch_passes_and_every_single_fault_is_refused_untouched(handles, family):
    lib, P = native.load(), native._p
    args, outputs = F.FAMILIES[family][2]()
    g = Guarded(outputs, 0xA5)
    outs = [g.ptr(name) for name, _, _ in outputs]
    assert F.call(lib, P, family, handles, dict(args), outs) == 0
    g.check_guards(f"{family}: valid")
    assert not g.untouched(outputs[0][0])
    for fault, apply in F.FAULTS[family].items():
        a = dict(args)
        apply(a)
        g.refill()
        assert F.call(lib, P, family, handles, a, outs) == F.EXPECTED[family, fault], (family, fault)
        g.check_guards(f"{family}: {fault}")
        for name, _, _ in outputs:
            assert g.untouched(name), (family, fault, name)
