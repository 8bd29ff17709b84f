"""Dependency resolution of a downloaded transaction graph on the GPU engine.

Mirrors the body of ResolveTransactionsFlow.call over the transactions downloadDependencies returned:
  topologicalSort                        core/src/main/kotlin/net/corda/flows/ResolveTransactionsFlow.kt:37-67
    forwardGraph: input.txhash -> LinkedHashSet of the transactions that spend it, visit() in download order with
    the visited set, post-order, reversed, require(result.size == transactions.size)
  the loop                               ResolveTransactionsFlow.kt:105-111
    stx.toLedgerTransaction(serviceHub): verifySignatures() without allowed keys (SignedTransaction.kt:134), then
    every input through loadState (ServiceHub.kt:46-49): TransactionResolutionException when the dependency is not
    recorded, `outputs[stateRef.index]` out of range otherwise; ltx.verify(); recordTransactions
  the duplicate check                    ResolveTransactionsFlow.kt:170

`resolve_transactions(stxs, engine)` takes the downloads in download order (resultQ.values) and returns
(order, n_pass, exception): topologicalSort's list, how many of its leading transactions pass everything checked here
(the caller runs their contracts and records them) and the exception the reference would raise at the stop, or None.
fused=True makes ONE cv_resolve_batch call; fused=False is the composition it replaces — the Merkle call, the verify
call, the missing-signers call and this module's restatement of the graph work — kept as the comparison for tests and
tools/resolve_fused_bench.py.  Contract verification (ltx.verify), attachments, the storage lookup of inputs that are
not in the batch, the download loop with its count limit and the final single stx / wtx of :119-125 stay with the
caller.

An input of a WireTransaction here is the blob of a StateRef: the 32 bytes of txhash, then index as 4 big-endian
bytes (Kryo stays outside).
"""
from __future__ import annotations

import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import native
from .crypto import IllegalStateException, InvalidKeyException, SignatureException
from .transactions import (MerkleTreeException, SecureHash, SignedTransaction, _device_decidable, _missing_exception,
                           compute_ids, flatten_must_sign, flatten_signatures, must_sign_reqs, verify_signatures_batch)


class TransactionResolutionException(Exception):
    """net.corda.core.contracts.TransactionResolutionException(hash)"""

    def __init__(self, hash: SecureHash):
        super().__init__(f"Transaction resolution failure for {hash!r}")
        self.hash = hash


class StateRef:
    """StateRef(txhash, index) (core/.../contracts/Structures.kt); .blob is the input leaf of a WireTransaction."""
    __slots__ = ("txhash", "index")

    def __init__(self, txhash: SecureHash, index: int):
        self.txhash, self.index = txhash, int(index)

    @property
    def blob(self) -> bytes:
        return self.txhash.bytes + struct.pack(">I", self.index)

    @staticmethod
    def parse(blob: bytes) -> "StateRef":
        if len(blob) != 36:
            raise ValueError(f"a StateRef blob is 36 bytes, not {len(blob)}")
        return StateRef(SecureHash(blob[:32]), struct.unpack(">I", blob[32:])[0])

    def __eq__(self, other):
        return isinstance(other, StateRef) and (other.txhash, other.index) == (self.txhash, self.index)

    def __hash__(self):
        return hash((self.txhash, self.index))

    def __repr__(self):
        return f"{self.txhash!r}({self.index})"


def _inputs(stx: SignedTransaction) -> List[StateRef]:
    return [StateRef.parse(b) for b in stx._wtx.inputs]


def topological_sort(stxs: Sequence[SignedTransaction]) -> List[SignedTransaction]:
    """topologicalSort (:37-67), with an explicit stack where the reference recurses."""
    forward: Dict[SecureHash, Dict[int, SignedTransaction]] = {}     # a dict keeps insertion order: the LinkedHashSet
    for tx in stxs:
        for ref in _inputs(tx):
            forward.setdefault(ref.txhash, {}).setdefault(id(tx), tx)
    visited = set()
    result: List[SignedTransaction] = []
    for root in stxs:
        if root.id in visited:
            continue
        visited.add(root.id)
        stack = [(root, iter(forward.get(root.id, {}).values()))]
        while stack:
            tx, it = stack[-1]
            nxt = next(it, None)
            if nxt is None:
                result.append(tx)
                stack.pop()
            elif nxt.id not in visited:
                visited.add(nxt.id)
                stack.append((nxt, iter(forward.get(nxt.id, {}).values())))
    result.reverse()
    if len(result) != len(stxs):
        raise IllegalStateException("Failed requirement.")
    return result


def _resolve_composed(stxs: Sequence[SignedTransaction], engine) -> Tuple[list, int, Optional[Exception]]:
    """The existing calls and the restatement: ids (one Merkle call), the `tx` getter of every download, the duplicate
    check, topological_sort, verifySignatures of all (one verify call, one missing-signers call), then the loop."""
    unknown = [s._wtx for s in stxs if s._wtx._id is None]
    if unknown:
        compute_ids(unknown, engine)
    for stx in stxs:                                                   # :167 / :41 touch stx.tx of every download
        if not stx._wtx.leaves:
            return [], 0, MerkleTreeException("Cannot calculate Merkle root on empty hash list.")
        try:
            stx.tx
        except IllegalStateException as e:
            return [], 0, e
    seen = set()
    for stx in stxs:                                                   # :170
        if stx.id in seen:
            return [], 0, IllegalStateException("Check failed.")
        seen.add(stx.id)
    order = topological_sort(stxs)
    errs = verify_signatures_batch(stxs, engine=engine, device_signers=True)
    err_of = {id(s): e for s, e in zip(stxs, errs)}
    by_id = {s.id: s for s in stxs}
    recorded = set()
    for n, stx in enumerate(order):
        if err_of[id(stx)] is not None:
            return order, n, err_of[id(stx)]
        for ref in _inputs(stx):                                       # loadState, input by input
            dep = by_id.get(ref.txhash)
            if dep is None:
                continue                                               # not downloaded: the node stores it already
            if ref.txhash not in recorded:
                return order, n, TransactionResolutionException(ref.txhash)
            if ref.index >= len(dep._wtx.outputs):
                return order, n, IndexError(f"Index: {ref.index}, Size: {len(dep._wtx.outputs)}")
        recorded.add(stx.id)
    return order, len(order), None


def flatten_resolve(stxs: Sequence[SignedTransaction]):
    """The arrays of Engine.resolve_batch for stxs -> (args by name, pre_err: the host prefilter's exception by
    absolute signature index)."""
    leaves: List[bytes] = []
    txb, tib, hashes, index, nout = [0], [0], [], [], []
    for stx in stxs:
        w = stx._wtx
        leaves.extend(w.leaves)
        txb.append(len(leaves))
        for ref in _inputs(stx):
            hashes.append(ref.txhash.bytes)
            index.append(ref.index)
        tib.append(len(index))
        nout.append(len(w.outputs))
    arena, offs, lens = native.pack_blobs(leaves)
    sigs, keys, pre_err = flatten_signatures(stxs)
    args = dict(arena=arena, leaf_off=offs, leaf_len=lens, tx_leaf_begin=np.array(txb, np.uint32),
                claimed_id=np.frombuffer(b"".join(s.id.bytes for s in stxs), np.uint8).reshape(-1, 32),
                sigs=sigs, reqs=must_sign_reqs(flatten_must_sign(stxs), keys, allowed=False),
                tx_input_begin=np.array(tib, np.uint32),
                input_txhash=np.frombuffer(b"".join(hashes), np.uint8).reshape(-1, 32),
                input_index=np.array(index, np.uint32), tx_output_count=np.array(nout, np.uint32))
    return args, pre_err


def _resolve_fused(stxs: Sequence[SignedTransaction], engine) -> Tuple[list, int, Optional[Exception]]:
    for stx in stxs:
        if not all(_device_decidable(k) for k in stx._wtx.must_sign):
            raise ValueError("fused resolve: a mustSign entry that the device cannot decide")
    args, pre_err = flatten_resolve(stxs)
    out = engine.resolve_batch(**args)
    g = dict(zip(native.RG_WORDS, (int(v) for v in out["graph"])))
    for k, stx in enumerate(stxs):
        if out["outcome"][k] != native.CV_RS_EMPTY and stx._wtx._id is None:
            stx._wtx._id = SecureHash(out["ids"][k].tobytes())
    if (out["outcome"] == native.CV_RS_MALFORMED).any():
        raise IllegalStateException("cv_resolve_batch: the flattened mustSign trees came back malformed")
    if g["status"] == native.CV_RG_BAD_ID:
        stx = stxs[g["which"]]
        if out["outcome"][g["which"]] == native.CV_RS_EMPTY:
            return [], 0, MerkleTreeException("Cannot calculate Merkle root on empty hash list.")
        try:
            stx.tx
            raise IllegalStateException("cv_resolve_batch: an id mismatch the mirror does not see")
        except IllegalStateException as e:
            return [], 0, e
    if g["status"] == native.CV_RG_DUPLICATE_ID:
        return [], 0, IllegalStateException("Check failed.")
    order = [stxs[int(t)] for t in out["order"]]
    cls, t, i = g["stop_class"], g["stop_tx"], g["stop_input"]
    if cls == native.RS_NONE:
        return order, g["n_pass"], None
    stx = stxs[t]
    if cls in (native.CV_RS_TX_INVALID, native.CV_RS_BAD_KEY):
        bad = int(out["first_bad"][t])
        e = pre_err.get(bad) or (InvalidKeyException("not a valid GroupElement") if cls == native.CV_RS_BAD_KEY
                                 else SignatureException("Signature did not match"))
    elif cls == native.CV_RS_SIGNATURES_MISSING:
        trb = args["reqs"][7]
        b, end = int(trb[t]), int(trb[t + 1])
        e = _missing_exception(stx, {stx._wtx.must_sign[j] for j in range(end - b) if out["req_missing"][b + j] == 1})
    elif cls == native.CV_RS_UNRESOLVED:
        e = TransactionResolutionException(SecureHash(args["input_txhash"][i].tobytes()))
    elif cls == native.CV_RS_BAD_INPUT:
        dep = stxs[int(out["input_dep"][i])]
        e = IndexError(f"Index: {int(args['input_index'][i])}, Size: {len(dep._wtx.outputs)}")
    else:
        raise IllegalStateException(f"cv_resolve_batch: stop class {cls}")
    return order, g["n_pass"], e


def resolve_transactions(stxs: Sequence[SignedTransaction], engine: Optional[native.Engine] = None, fused: bool = True
                         ) -> Tuple[List[SignedTransaction], int, Optional[Exception]]:
    """The body of ResolveTransactionsFlow.call over the downloads stxs, in download order -> (order, n_pass,
    exception), see the module's header.  The exceptions: MerkleTreeException / IllegalStateException (a download whose
    id cannot be computed or does not match, a duplicate id: order is empty), SignatureException, InvalidKeyException,
    SignaturesMissingException, TransactionResolutionException, IndexError."""
    stxs = list(stxs)
    if not stxs:
        return [], 0, None
    eng = engine or native.default_engine()
    return _resolve_fused(stxs, eng) if fused else _resolve_composed(stxs, eng)
