"""The outputs of cv_resolve_batch under the header's Conventions (include/cordaverify.h): every output carved by
tests/guarded.py at the alignment of its C type and no more, poisoned and guard-banded.  A successful call writes every
byte of every output it is given and nothing around it, whatever they held; each optional output may be NULL; order is
zero-filled for a batch with a duplicate id whatever the buffer held before.  Two poison bytes, so a result ORed into
what was there shows.
"""
import numpy as np
import pytest

import resolve_cases as C
from corda_amd import native
from guarded import Guarded

pytestmark = pytest.mark.gpu

OPTIONAL = ("first_bad", "req_missing", "ids")


@pytest.fixture(scope="module")
def batches(engine, corpus):
    """A batch per size — every fault the size has room for along a chain, an out-of-range input, outside inputs —
    one with a duplicate id, and what the call returns for them into fresh arrays."""
    memo = {}

    def get(n, dup=False):
        if (n, dup) not in memo:
            specs = C.chain(n)
            for t, f in ((3, "bad_sig"), (9, "missing"), (20, "bad_key"), (33, "malformed"), (50, "nosig")):
                if t < n:
                    specs[t]["faults"] = {f}
            if n > 40:
                specs[40]["inputs"] = [(41, 1), ("x", 0)]
            if dup:
                specs[n - 1]["same_as"] = 5
            b = C.real(engine, corpus, specs)
            memo[n, dup] = (b, engine.resolve_batch(**b, seed=5))
        return memo[n, dup]
    return get


def call(engine, b, g, absent=()):
    lib, P = native.load(), native._p
    pk, sig, tsb, _ = b["sigs"]
    ntx, nin = len(b["tx_output_count"]), len(b["input_index"])
    reqs = b["reqs"]
    nreq, nnodes, nchild = len(reqs[6]) - 1, len(reqs[3]) - 1, len(reqs[4])
    outs = [None if k in absent else g.ptr(k) for k in native.Engine.RESOLVE_OUTPUTS]
    return lib.cv_resolve_batch(engine._h, ntx, P(b["arena"]), b["arena"].size, P(b["leaf_off"]), P(b["leaf_len"]),
                                P(b["tx_leaf_begin"]), P(b["claimed_id"]), P(pk), P(sig), P(tsb), None, nreq, nnodes, nchild,
                                *[P(a) if a.size else None for a in reqs], nin, P(b["tx_input_begin"]), P(b["input_txhash"]),
                                P(b["input_index"]), P(b["tx_output_count"]), 5, *outs)


def spec_of(b):
    ntx, nin, nreq = len(b["tx_output_count"]), len(b["input_index"]), len(b["reqs"][6]) - 1
    return [("outcome", ntx, 1), ("first_bad", 4 * ntx, 4), ("req_missing", nreq, 1), ("bad_input", 4 * ntx, 4),
            ("input_dep", 4 * nin, 4), ("input_status", nin, 1), ("order", 4 * ntx, 4), ("graph", 4 * len(C.G_WORDS), 4),
            ("ids", 32 * ntx, 1)]


DTYPE = {"first_bad": np.uint32, "bad_input": np.uint32, "input_dep": np.uint32, "order": np.uint32, "graph": np.uint32}


def check(g, want, absent, what):
    g.check_guards(what)
    for k in native.Engine.RESOLVE_OUTPUTS:
        if k in absent:
            assert g.untouched(k), (what, k)
        else:
            got = g.read(k, DTYPE.get(k, np.uint8))
            assert np.array_equal(got, want[k].reshape(-1)), (what, k)


@pytest.mark.parametrize("fill", (0x00, 0xA5))
@pytest.mark.parametrize("n", (1, 64, 65, 1025))
def test_outputs_written_whole_and_nothing_around(engine, batches, n, fill):
    b, want = batches(n)
    g = Guarded(spec_of(b), fill)
    assert call(engine, b, g) == 0
    check(g, want, (), f"n {n} fill {fill:#x}")


@pytest.mark.parametrize("absent", OPTIONAL + (OPTIONAL,))
def test_each_optional_output_absent(engine, batches, absent):
    absent = (absent,) if isinstance(absent, str) else absent
    b, want = batches(65)
    g = Guarded(spec_of(b), 0xFF)
    assert call(engine, b, g, absent) == 0
    check(g, want, absent, f"absent {absent}")


@pytest.mark.parametrize("fill", (0x00, 0xFF, 0xA5))
def test_order_is_zero_filled_for_a_duplicate_id(engine, batches, fill):
    b, want = batches(65, dup=True)
    assert want["graph"][0] == C.G_DUPLICATE_ID and want["graph"][1] == 5 and want["graph"][2] == 0
    g = Guarded(spec_of(b), fill)
    assert call(engine, b, g) == 0
    check(g, want, (), f"duplicate fill {fill:#x}")
    assert not g.read("order", np.uint32).any()
