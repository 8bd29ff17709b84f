"""cv_missing_signers on the GPU (corda_amd/csrc/cv_k_ck.hip): every case of tests/ck_cases.py through the host form
with the three wide_min values, equal to fulfilled_ref and the status rule; the device form on torch tensors chained
on one stream behind cv_ed25519_verify_device over real signatures of the golden corpus; and the mirror's opt-in
wiring (verify_signatures_batch, its fused form and BatchingNotary with device_signers=True) against the same calls
with the option off, result for result and exception field for exception field.  Every comparison is exact.
"""
import numpy as np
import pytest
import torch

import ck_cases as C
from corda_amd import native
from corda_amd.crypto import CompositeKey, DigitalSignature, DummyPublicKey, EdDSAPublicKey
from corda_amd.notary import BatchingNotary, SignRequest
from corda_amd.transactions import (SignaturesMissingException, SignedTransaction, WireTransaction, compute_ids,
                                    missing_signatures_batch, verify_signatures_batch, verify_signatures_batch_fused)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLAT = ("kind", "leaf_key", "threshold", "child_begin", "child", "weight", "req_begin", "tx_req_begin", "sig_key",
        "tx_sig_begin")


@pytest.fixture(scope="module")
def built():
    return {name: C.build(make()) for name, make in C.CASES.items()}


@pytest.mark.parametrize("wide_min", C.WIDE_MINS)
def test_every_case_host_form(engine, built, wide_min):
    for name, (f, want_missing, want_status) in built.items():
        rm, st = engine.missing_signers(*[f[k] for k in FLAT], req_allowed=f["req_allowed"], bitmap=f["bitmap"],
                                        wide_min=wide_min)
        assert rm.tolist() == want_missing.tolist(), (name, wide_min)
        assert st.tolist() == want_status.tolist(), (name, wide_min)


def test_req_allowed_null_means_none(engine, built):
    f, want_missing, _ = built["req_allowed"]
    rm, st = engine.missing_signers(*[f[k] for k in FLAT])
    assert rm.tolist() == want_missing.tolist()
    trb = f["tx_req_begin"]
    assert st.tolist() == [C.VS_MISSING if (want_missing[trb[t]:trb[t + 1]] == 1).any() else C.VS_OK for t in range(len(trb) - 1)]


@pytest.mark.parametrize("wide_min", C.WIDE_MINS)
def test_no_requirements_at_all(engine, wide_min):
    """nreq = nnodes = nchild = 0, with req_allowed and verdict_bitmap NULL and with both given."""
    f, want_missing, want_status = C.build(C.no_requirements())
    assert f["kind"].size == 0 and want_missing.size == 0 and want_status.tolist() == [C.VS_OK, C.VS_BAD_SIGNATURE, C.VS_OK]
    nsig = int(f["tx_sig_begin"][-1])
    for opt in ({}, {"req_allowed": f["req_allowed"], "bitmap": C.all_ones(nsig)}):
        rm, st = engine.missing_signers(*[f[k] for k in FLAT], wide_min=wide_min, **opt)
        assert rm.size == 0 and st.tolist() == want_status.tolist(), (wide_min, sorted(opt))
    f, _, want_status = C.build(C.Case(C.no_requirements().txs, bitmap=C.ones_except(1)))   # the last one's first signature
    _, st = engine.missing_signers(*[f[k] for k in FLAT], bitmap=f["bitmap"], wide_min=wide_min)
    assert st.tolist() == want_status.tolist() == [C.VS_OK, C.VS_BAD_SIGNATURE, C.VS_BAD_SIGNATURE]


def _up(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(DEV)


def test_device_form_behind_verify_on_one_stream(engine, corpus):
    """About 200 corpus signatures, accepted and rejected ones mixed (the corpus's verdict column is the reference),
    as the signatures of transactions of 1 to 4; cv_ed25519_verify_device writes d_bitmap and cv_missing_signers_device
    reads it as it stands, both enqueued on one stream with no synchronisation between.  tx_status = what
    cv_tx_verdicts over the corpus verdicts plus the host mirror's is_fulfilled_by give."""
    rng = np.random.default_rng(5)
    acc, rej = np.nonzero(corpus["verdict"] == 1)[0], np.nonzero(corpus["verdict"] == 0)[0]
    rows = np.concatenate([rng.choice(acc, 170, replace=len(acc) < 170), rng.choice(rej, 30, replace=len(rej) < 30)])
    rng.shuffle(rows)
    n = len(rows)
    pks = [EdDSAPublicKey(corpus["pk"][r].tobytes()) for r in rows]
    txs, s = [], 0
    while s < n:
        m = min(int(rng.integers(1, 5)), n - s)
        mine = pks[s:s + m]
        stranger = C.key("dev-stranger", s)
        shape = len(txs) % 4
        if shape == 0:
            ms = [C.Leaf(k) for k in mine]
        elif shape == 1:
            ms = [C.Leaf(mine[0]), C.Leaf(stranger)]
        elif shape == 2:
            ms = [C.node(1, [C.Leaf(stranger), C.Leaf(mine[-1])]), C.node(2, [C.Leaf(stranger), C.Leaf(mine[0])])]
        else:
            ms = [C.node(m, [C.Leaf(k) for k in mine])]
        txs.append(C.Tx(ms, mine, [ms[-1]] if len(txs) % 3 == 0 else []))
        s += m
    f = C.flatten(txs)
    ntx, nreq, nnodes, nchild = len(txs), f["req_begin"].size - 1, f["kind"].size, f["child"].size
    # the expectation: the corpus verdicts through cv_tx_verdicts, then the mirror
    want_bits = np.packbits(corpus["verdict"][rows].astype(bool), bitorder="little")
    want_bm = np.zeros((n + 63) // 64, np.uint64)
    want_bm.view(np.uint8)[:want_bits.size] = want_bits
    ok = native.tx_verdicts(want_bm, f["tx_sig_begin"])
    want_missing, want_status = [], []
    for t, tx in enumerate(txs):
        miss = [not r.is_fulfilled_by(set(tx.signers)) for r in tx.must_sign]
        want_missing += [int(x) for x in miss]
        need = any(x and r not in tx.allowed for x, r in zip(miss, tx.must_sign))
        want_status.append(C.VS_BAD_SIGNATURE if not ok[t] else C.VS_MISSING if need else C.VS_OK)
    assert {C.VS_OK, C.VS_BAD_SIGNATURE, C.VS_MISSING} == set(want_status)
    d = {k: _up(f[k]) for k in FLAT + ("req_allowed",)}
    v = {"pk": _up(corpus["pk"][rows]), "sig": _up(corpus["sig"][rows]), "arena": _up(corpus["arena"]),
         "off": _up(corpus["off"][rows].astype(np.uint64)), "len": _up(corpus["len"][rows].astype(np.uint32))}
    ws_bytes = native.missing_signers_workspace(ntx, nnodes)
    stream = torch.cuda.Stream(DEV)
    for wide_min in C.WIDE_MINS:
        bitmap = torch.full((8 * ((n + 63) // 64),), 0xA5, dtype=torch.uint8, device=DEV)
        rm = torch.full((nreq,), 0xEE, dtype=torch.uint8, device=DEV)
        st = torch.full((ntx,), 0xEE, dtype=torch.uint8, device=DEV)
        ws = torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        engine.verify_device(0, n, v["pk"].data_ptr(), v["sig"].data_ptr(), v["arena"].data_ptr(), v["off"].data_ptr(),
                             v["len"].data_ptr(), bitmap.data_ptr(), 0, stream.cuda_stream)
        engine.missing_signers_device(0, ntx, nreq, nnodes, nchild, n, *[d[k].data_ptr() for k in FLAT],
                                      d["req_allowed"].data_ptr(), bitmap.data_ptr(), wide_min, rm.data_ptr(),
                                      st.data_ptr(), ws.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(bitmap.cpu().numpy().view(np.uint64), want_bm), wide_min
        assert rm.cpu().numpy().tolist() == want_missing, wide_min
        assert st.cpu().numpy().tolist() == want_status, wide_min


# ---------------------------------------------------------------- the mirror's opt-in wiring
def _mixed_batch(engine, n=300):
    """n signed transactions: valid ones, a corrupted signature, a missing signer, a missing signer that is allowed
    (the notary key), composite requirements, a DummyPublicKey requirement (decided on the host), a mismatched id."""
    seeds = np.frombuffer(b"".join(bytes([i % 251 + 1, i // 251 + 1]) * 16 for i in range(8)), np.uint8).reshape(8, 32)
    notary_key = BatchingNotary(bytes([21]) * 32, engine=engine).owning_key
    probe = np.zeros(16, np.uint8)
    pk8, _ = engine.sign_batch(seeds, probe, np.zeros(8, np.uint64), np.zeros(8, np.uint32))
    keys = [EdDSAPublicKey(pk8[i].tobytes()) for i in range(8)]
    leaves = [k.composite for k in keys]
    wtxs, signers = [], []
    for t in range(n):
        a, b, c = t % 8, (t + 3) % 8, (t + 5) % 8
        kind = t % 10
        must = [leaves[a], leaves[b], CompositeKey.Node(1, [leaves[c], leaves[(c + 1) % 8]], [1, 1])]
        sg = [a, b, c]
        if kind == 3:
            sg = [a, c]                                            # leaves[b] missing
        elif kind == 4:
            must = must + [notary_key]                             # missing, and what the notary allows
        elif kind == 5:
            must = [leaves[a], notary_key, leaves[b]]
            sg = [a]                                               # one missing allowed, one not
        elif kind == 6:
            must = must + [CompositeKey.Leaf(DummyPublicKey(f"dummy-{t}"))]   # decided on the host, as before
        elif kind == 7:
            must = [CompositeKey.Node(3, [leaves[a], leaves[b], leaves[c]], [2, 2, -1])]   # 2 + 2 - 1 = 3
            sg = [a, b, c] if t % 20 == 7 else [a, b]
        wtx = WireTransaction(inputs=[b"in-%d" % t], outputs=[b"out"], commands=[b"cmd"], must_sign=must,
                              command_descriptions={m: f"cmd-{t}-{i}" for i, m in enumerate(must)},
                              notary_key=notary_key if kind in (4, 5) else None)
        wtxs.append(wtx)
        signers.append(sg)
    compute_ids(wtxs, engine)
    flat = [(t, s) for t in range(n) for s in signers[t]]
    arena = np.frombuffer(b"".join(wtxs[t]._id.bytes for t, _ in flat), np.uint8)
    _, sig = engine.sign_batch(seeds[[s for _, s in flat]], arena, np.arange(len(flat), dtype=np.uint64) * 32,
                               np.full(len(flat), 32, np.uint32))
    stxs, j = [], 0
    for t in range(n):
        sigs = []
        for s in signers[t]:
            bits = sig[j].tobytes()
            if t % 10 == 8 and s == signers[t][-1]:
                bits = bytes([bits[0] ^ 1]) + bits[1:]             # a corrupted signature
            sigs.append(DigitalSignature.WithKey(keys[s], bits))
            j += 1
        wtx = wtxs[t]
        if t % 50 == 9:                                            # contents that are not the signed id's
            wtx = WireTransaction(inputs=wtx.inputs, outputs=[b"changed"], commands=wtx.commands, must_sign=wtx.must_sign)
        stxs.append(SignedTransaction(wtx, sigs, wtxs[t]._id))
    return stxs, notary_key


def _same_exception(x, y, what):
    assert type(x) is type(y), what
    if x is None:
        return
    if isinstance(x, SignaturesMissingException):     # (the message lists the set in its iteration order)
        assert x.missing == y.missing and x.descriptions == y.descriptions and x.id == y.id, what
    else:
        assert str(x) == str(y), what


@pytest.fixture(scope="module")
def mixed(engine):
    return _mixed_batch(engine)


def test_mirror_batch_verify_with_device_signers(engine, mixed):
    stxs, notary_key = mixed
    for fn in (verify_signatures_batch, verify_signatures_batch_fused):
        for allowed in ((), (notary_key,)):
            off = fn(stxs, allowed, engine)
            on = fn(stxs, allowed, engine, device_signers=True)
            assert len(off) == len(on) == len(stxs)
            for k, (x, y) in enumerate(zip(off, on)):
                _same_exception(x, y, (fn.__name__, len(allowed), k))
            kinds = {type(x).__name__ for x in off}
            assert {"NoneType", "SignaturesMissingException", "SignatureException", "IllegalStateException"} <= kinds


def test_missing_signatures_batch_is_the_mirror(engine, mixed):
    stxs, notary_key = mixed
    got = missing_signatures_batch(stxs, (notary_key,), engine)
    for k, stx in enumerate(stxs):
        missing = {r for r in stx._wtx.must_sign if not r.is_fulfilled_by({s.by for s in stx.sigs})} - {notary_key}
        assert (got[k] is None) == (not missing), k
        if missing:
            assert got[k].missing == missing and got[k].id == stx.id


def test_notary_with_device_signers(engine, mixed):
    stxs, _ = mixed
    reqs = [SignRequest(s, f"party-{k % 7}") for k, s in enumerate(stxs)]
    res = [BatchingNotary(bytes([21]) * 32, validating=True, engine=engine, device_signers=flag).notarise(reqs)
           for flag in (False, True)]
    assert len(res[0]) == len(res[1]) == len(stxs)
    for k, (x, y) in enumerate(zip(*res)):
        assert x.ok == y.ok and type(x.error) is type(y.error) and type(x.failure) is type(y.failure), k
        if x.ok:
            assert x.sig.bits == y.sig.bits and x.sig.by == y.sig.by, k
        if getattr(x.error, "missing_signers", None) is not None:
            assert x.error.missing_signers == y.error.missing_signers, k
        if x.failure is not None:
            assert str(x.failure) == str(y.failure), k
    assert {type(x.error).__name__ for x in res[0]} >= {"NoneType", "SignaturesMissing", "TransactionInvalid"}
