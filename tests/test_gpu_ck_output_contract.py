"""The output contract of cv_missing_signers and cv_missing_signers_device (include/cordaverify.h, Conventions): the
outputs may hold anything on entry and every byte of req_missing and tx_status is written, nothing before or behind
them is, the device form's workspace is used inside cv_missing_signers_workspace bytes, ntx == 0 writes nothing, and
the inputs are only read.  Outputs are carved from poisoned, guard-banded allocations (tests/guarded.py) at odd
addresses, the workspace at 16 mod 32; the values are compared with tests/ck_cases.py's oracle, exactly.

Sizes: ntx and nreq at 1 and around CV_BLOCK (255, 256, 257) — together, and one of them large beside the other at 1.
"""
import numpy as np
import pytest
import torch

import ck_cases as C
from corda_amd import native
from guarded import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILLS = (0x00, 0xFF)
FLAT = ("kind", "leaf_key", "threshold", "child_begin", "child", "weight", "req_begin", "tx_req_begin", "sig_key",
        "tx_sig_begin")
SHAPES = [(1, 1), (255, 255), (256, 256), (257, 257), (1, 257), (257, 1)]          # (ntx, nreq)


def _case(ntx, nreq):
    """ntx transactions owning nreq requirements (one each, or all with the first one), a third missing, some
    composite, some allowed; one transaction without signers where there are several."""
    pool = [C.key("oc", i) for i in range(7)]
    reqs = []
    for r in range(nreq):
        x, y = C.Leaf(pool[r % 7]), C.Leaf(pool[(r + 2) % 7])
        reqs.append(x if r % 3 else C.node(2, [x, y]))
    txs = []
    for t in range(ntx):
        mine = reqs if ntx == 1 else reqs[t:t + 1] if nreq > 1 else (reqs if t == 0 else [])
        signers = [] if (t == 5) else [pool[t % 7], pool[(t + 1) % 7]]
        txs.append(C.Tx(list(mine), signers, [mine[0]] if mine and t % 4 == 0 else []))
    return C.Case(txs, bitmap=C.ones_except(*range(3, 2 * ntx, 11)))


@pytest.fixture(scope="module")
def built():
    out = {}
    for shape in SHAPES:
        f, rm, st = C.build(_case(*shape))
        assert (len(st), len(rm)) == shape
        out[shape] = (f, rm, st)
    return out


def _counts(f):
    return (f["tx_req_begin"].size - 1, f["req_begin"].size - 1, f["kind"].size, f["child"].size, f["sig_key"].shape[0])


def _pad(a):
    return a if a.size else np.zeros((1,) + a.shape[1:], a.dtype)


@pytest.mark.parametrize("wide_min", C.WIDE_MINS)
def test_host_form_outputs(engine, built, wide_min):
    lib = native.load()
    for shape, (f, want_rm, want_st) in built.items():
        ntx, nreq, nnodes, nchild, nsig = _counts(f)
        ins = [_pad(f[k]) for k in FLAT] + [f["req_allowed"], f["bitmap"]]
        before = [a.copy() for a in ins]
        for fill in FILLS:
            g = Guarded([("req_missing", nreq, 1), ("tx_status", ntx, 1)], fill)
            rc = lib.cv_missing_signers(engine._h, ntx, nreq, nnodes, nchild, nsig, *[native._p(a) for a in ins], wide_min,
                                        g.ptr("req_missing"), g.ptr("tx_status"))
            what = ("host", shape, wide_min, hex(fill))
            assert rc == 0, what
            assert g.read("req_missing").tolist() == want_rm.tolist(), what
            assert g.read("tx_status").tolist() == want_st.tolist(), what
            g.check_guards(str(what))
        for a, b in zip(ins, before):
            assert np.array_equal(a, b), (shape, "an input was written")


def test_host_form_empty_call_writes_nothing(engine):
    lib = native.load()
    g = Guarded([("req_missing", 8, 1), ("tx_status", 8, 1)], 0x3C)
    assert lib.cv_missing_signers(engine._h, 0, 0, 0, 0, 0, *[None] * 12, 0, g.ptr("req_missing"), g.ptr("tx_status")) == 0
    assert g.untouched("req_missing") and g.untouched("tx_status")
    g.check_guards("ntx == 0")


def _up(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(DEV)


@pytest.mark.parametrize("wide_min", C.WIDE_MINS)
def test_device_form_outputs(engine, built, wide_min):
    own = torch.cuda.Stream(DEV)
    for shape, (f, want_rm, want_st) in built.items():
        ntx, nreq, nnodes, nchild, nsig = _counts(f)
        d = {k: _up(_pad(f[k])) for k in FLAT}
        d["req_allowed"], d["bitmap"] = _up(f["req_allowed"]), _up(f["bitmap"])
        orig = {k: v.clone() for k, v in d.items()}
        ws_bytes = native.missing_signers_workspace(ntx, nnodes)
        for fill in FILLS:
            for stream in (0, own.cuda_stream):
                g = Guarded([("req_missing", nreq, 1), ("tx_status", ntx, 1), ("workspace", ws_bytes, 16)], fill, device=DEV)
                torch.cuda.synchronize()
                engine.missing_signers_device(0, ntx, nreq, nnodes, nchild, nsig, *[d[k].data_ptr() for k in FLAT],
                                              d["req_allowed"].data_ptr(), d["bitmap"].data_ptr(), wide_min,
                                              g.ptr("req_missing"), g.ptr("tx_status"), g.ptr("workspace"), stream)
                torch.cuda.synchronize()
                what = ("device", shape, wide_min, hex(fill), "own stream" if stream else "context stream")
                g.snapshot()
                assert g.read("req_missing").tolist() == want_rm.tolist(), what
                assert g.read("tx_status").tolist() == want_st.tolist(), what
                g.check_guards(str(what))              # the workspace's guard bands included
        for k in d:
            assert torch.equal(d[k], orig[k]), (shape, f"input {k} was written")


def test_device_form_empty_call_writes_nothing(engine):
    g = Guarded([("req_missing", 8, 1), ("tx_status", 8, 1), ("workspace", 64, 16)], 0x3C, device=DEV)
    torch.cuda.synchronize()
    engine.missing_signers_device(0, 0, 0, 0, 0, 0, *[0] * 12, 0, g.ptr("req_missing"), g.ptr("tx_status"),
                                  g.ptr("workspace"))
    torch.cuda.synchronize()
    g.snapshot()
    assert g.untouched("req_missing") and g.untouched("tx_status") and g.untouched("workspace")
    g.check_guards("ntx == 0")
