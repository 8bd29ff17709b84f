"""The binding's marshalling helpers, which need neither the library nor a device: native._arr, _sig_args, _req_args
and pack_blobs, and transactions.flatten_signatures.  Empty inputs yield the one-element placeholders the library is
handed (never a NULL for an empty array), size mismatches raise ValueError, the tear-off calls' lenient form passes
longer arrays.
"""
import numpy as np
import pytest

from corda_amd import native
from corda_amd.crypto import EdDSAPublicKey, InvalidKeyException, SignatureException
from corda_amd.native import _arr, _req_args, _sig_args, pack_blobs
from corda_amd.transactions import flatten_signatures, must_sign_reqs

u32 = lambda *a: np.array(a, np.uint32)      # noqa: E731
NONE32 = np.zeros((0, 32), np.uint8)


def test_arr_shapes_placeholders_and_mismatches():
    a = _arr([[1, 2], [3, 4]], np.uint32, 2, "x", 2)
    assert a.dtype == np.uint32 and a.tolist() == [1, 2, 3, 4] and a.flags.c_contiguous
    for width in (1, 32, 64):
        p = _arr([], np.uint8, 0, "x", width)
        assert p.dtype == np.uint8 and p.size == width and not p.any()
    for n in (1, 3):                                     # exact: neither shorter nor longer
        with pytest.raises(ValueError, match="x must have %d entries, not 2" % n):
            _arr([7, 8], np.uint32, n, "x")
    with pytest.raises(ValueError, match="k must have 64 entries, not 32"):
        _arr(np.zeros(32, np.uint8), np.uint8, 2, "k", 32)
    # the tear-off calls' form: at least n rows
    assert _arr([7, 8, 9], np.uint32, 2, "x", exact=False).tolist() == [7, 8, 9]
    assert _arr([], np.uint32, 0, "x", exact=False).tolist() == [0]
    with pytest.raises(ValueError, match="x must have 4 entries, not 3"):
        _arr([7, 8, 9], np.uint32, 4, "x", exact=False)


def test_pack_blobs_equals_its_restatement():
    blobs = [bytes(range(n)) for n in (0, 1, 15, 16, 17)] + [b"", b"z"]
    arena, off, ln = pack_blobs(blobs)
    lens = [len(b) for b in blobs]
    assert ln.dtype == np.uint32 and ln.tolist() == lens
    assert off.dtype == np.uint64 and off.tolist() == [sum(lens[:i]) for i in range(len(blobs))]
    assert arena.dtype == np.uint8 and arena.tobytes() == b"".join(blobs) + bytes(16)
    for b, o, n in zip(blobs, off, ln):
        assert arena[int(o):int(o) + int(n)].tobytes() == b
    arena, off, ln = pack_blobs([])                      # no blobs: empty offsets and lengths, the arena's tail alone
    assert off.shape == (0,) and off.dtype == np.uint64 and ln.shape == (0,) and ln.dtype == np.uint32
    assert arena.tobytes() == bytes(16)
    arena, off, ln = pack_blobs([b"abc"])
    assert off.tolist() == [0] and ln.tolist() == [3] and arena.size == 19


def test_sig_args():
    pk, sg = np.arange(64, dtype=np.uint8).reshape(2, 32), np.arange(128, dtype=np.uint8).reshape(2, 64)
    a, nsig = _sig_args((pk, sg, [0, 2, 2], [0, 1]), 2)
    assert nsig == 2 and [x.dtype for x in a] == [np.uint8, np.uint8, np.uint32, np.uint8]
    assert a[0].shape == (64,) and a[1].shape == (128,) and a[2].tolist() == [0, 2, 2] and a[3].tolist() == [0, 1]
    assert _sig_args((pk, sg, [0, 2, 2], None), 2)[0][3] is None
    a, nsig = _sig_args((NONE32, np.zeros((0, 64), np.uint8), [0, 0], np.zeros(0, np.uint8)), 1)     # no signatures
    assert nsig == 0 and [x.size for x in a] == [32, 64, 2, 1] and not any(x.any() for x in a)
    with pytest.raises(ValueError, match="tx_sig_begin must have 3 entries, not 2"):
        _sig_args((pk, sg, [0, 2], None), 2)
    with pytest.raises(ValueError, match="pk must have 96 entries, not 64"):
        _sig_args((pk, sg, [0, 2, 3], None), 2)
    with pytest.raises(ValueError, match="sig must have 128 entries, not 64"):
        _sig_args((pk, sg[:1], [0, 1, 2], None), 2)
    with pytest.raises(ValueError, match="sig_pre must have 2 entries, not 1"):
        _sig_args((pk, sg, [0, 1, 2], [0]), 2)


def _reqs(allowed=None):
    """Two requirements of two transactions: a leaf; a node of threshold 2 over two leaves."""
    r = ([0, 0, 0, 1], np.arange(128, dtype=np.uint8).reshape(4, 32), [0, 0, 0, 2], [0, 0, 0, 0, 2], [1, 2], [1, 1],
         [0, 1, 4], [0, 1, 2], np.zeros((3, 32), np.uint8))
    return r if allowed is None else r + (allowed,)


def test_req_args():
    a, nreq, nnodes, nchild = _req_args(_reqs(), 2, 3, allowed=False)
    assert (nreq, nnodes, nchild) == (2, 4, 2) and len(a) == 9
    assert [x.dtype for x in a] == [np.uint8, np.uint8, np.int32, np.uint32, np.uint32, np.int32, np.uint32, np.uint32,
                                    np.uint8]
    assert [x.size for x in a] == [4, 128, 4, 5, 2, 2, 3, 3, 96]
    a, *_ = _req_args(_reqs([1, 0]), 2, 3, allowed=True)
    assert len(a) == 10 and a[9].dtype == np.uint8 and a[9].tolist() == [1, 0]
    assert _req_args(_reqs(None) + (None,), 2, 3, allowed=True)[0][9] is None
    # nothing at all: zero requirements, nodes, children and signers -> one-element placeholders, the begins as given
    none = ([], NONE32, [], [0], [], [], [0], [0, 0], NONE32)
    a, nreq, nnodes, nchild = _req_args(none + ([],), 1, 0, allowed=True)
    assert (nreq, nnodes, nchild) == (0, 0, 0)
    assert [x.size for x in a] == [1, 32, 1, 1, 1, 1, 1, 2, 32, 1] and not any(x.any() for x in a)
    # leaves alone: nodes and no children
    a, nreq, nnodes, nchild = _req_args(([0], np.ones((1, 32), np.uint8), [0], [0, 0], [], [], [0, 1], [0, 1], NONE32), 1, 0,
                                        allowed=False)
    assert (nreq, nnodes, nchild) == (1, 1, 0) and a[4].tolist() == [0] and a[5].tolist() == [0] and a[8].size == 32
    r = list(_reqs())
    for i, n, what in ((0, 3, "kind must have 4 entries, not 3"), (1, 3, "leaf_key must have 128 entries, not 96"),
                       (2, 5, "threshold must have 4 entries, not 5"), (5, 1, "weight must have 2 entries, not 1"),
                       (7, 2, "tx_req_begin must have 3 entries, not 2")):
        bad = list(r)
        bad[i] = np.asarray(r[i])[:n] if n < len(r[i]) else list(r[i]) + [0]
        with pytest.raises(ValueError, match=what):
            _req_args(tuple(bad), 2, 3, allowed=False)
    with pytest.raises(ValueError, match="sig_key must have 128 entries, not 96"):
        _req_args(_reqs(), 2, 4, allowed=False)
    with pytest.raises(ValueError, match="req_allowed must have 2 entries, not 3"):
        _req_args(_reqs([0, 0, 0]), 2, 3, allowed=True)
    for i in (3, 6):                                     # child_begin, req_begin without their first entry
        bad = list(r)
        bad[i] = []
        with pytest.raises(ValueError, match="the begin arrays must have count \\+ 1 entries"):
            _req_args(tuple(bad), 2, 3, allowed=False)
    with pytest.raises(ValueError):                      # allowed: the tuple has ten entries
        _req_args(_reqs(), 2, 3, allowed=True)


class _Sig:
    def __init__(self, by, bits):
        self.by, self.bits = by, bits


class _Id:
    bytes = bytes(32)


class _Stx:
    id = _Id()

    def __init__(self, sigs):
        self.sigs = sigs


class _OtherKey:
    """A key that is not EdDSA: the prefilter's InvalidKeyException."""
    encoded = b"\x01" * 32


def test_flatten_signatures():
    k0, k1 = EdDSAPublicKey(bytes(range(32))), EdDSAPublicKey(bytes(range(1, 33)))
    good, short = bytes(range(64)), bytes(63)
    stxs = [_Stx([_Sig(k0, good), _Sig(k1, short)]), _Stx([]), _Stx([_Sig(_OtherKey(), good), _Sig(k1, good)])]
    sigs, keys, pre_err = flatten_signatures(stxs)
    pk, sg, tsb, sig_pre = sigs
    assert keys is pk and pk.shape == (4, 32) and sg.shape == (4, 64) and pk.dtype == sg.dtype == np.uint8
    assert tsb.dtype == np.uint32 and tsb.tolist() == [0, 2, 2, 4]
    assert sig_pre.dtype == np.uint8 and sig_pre.tolist() == [0, native.NS_PRE_SIGNATURE, native.NS_PRE_KEY, 0]
    assert sorted(pre_err) == [1, 2]
    assert isinstance(pre_err[1], SignatureException) and isinstance(pre_err[2], InvalidKeyException)
    assert pk[0].tobytes() == k0.encoded and pk[1].tobytes() == k1.encoded and pk[3].tobytes() == k1.encoded
    assert not pk[2].any()                               # a key that fails: zero bytes, and its signature's too
    assert sg[0].tobytes() == good and sg[3].tobytes() == good and not sg[1].any() and not sg[2].any()
    # no signature anywhere: empty rows, which the binding turns into its placeholders
    sigs, keys, pre_err = flatten_signatures([_Stx([]), _Stx([])])
    assert keys.shape == (0, 32) and sigs[1].shape == (0, 64) and sigs[2].tolist() == [0, 0, 0] and sigs[3].shape == (0,)
    assert pre_err == {}
    a, nsig = _sig_args(sigs, 2)
    assert nsig == 0 and [x.size for x in a] == [32, 64, 3, 1]
    sigs, keys, pre_err = flatten_signatures([])
    assert sigs[2].tolist() == [0] and keys.shape == (0, 32)


def test_must_sign_reqs_orders_the_dict():
    names = ("kind", "leaf_key", "threshold", "child_begin", "child", "weight", "req_begin", "tx_req_begin")
    f = {k: object() for k in names + ("sig_key", "tx_sig_begin", "req_allowed")}
    keys = object()
    assert must_sign_reqs(f, keys, allowed=False) == tuple(f[k] for k in names) + (keys,)
    assert must_sign_reqs(f, keys, allowed=True) == tuple(f[k] for k in names) + (keys, f["req_allowed"])
