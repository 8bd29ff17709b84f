"""Batched notary commit step on the GPU engine (BASELINE config C4 / SURVEY.md §8(a) a11).

The reference notarises one transaction per flow on the node's single thread:
  NotaryFlow.Service.call                core/src/main/kotlin/net/corda/flows/NotaryFlow.kt:96-113
    val wtx = stx.tx   (Merkle id recompute + check(temp.id == id), OUTSIDE the try: a mismatch is
                        an IllegalStateException that fails the flow, not a NotaryError)
    try { validateTimestamp -> beforeCommit -> commitInputStates -> sign(stx.id) }
    catch (NotaryException) -> Result.Error
  ValidatingNotaryFlow.beforeCommit      core/src/main/kotlin/net/corda/flows/ValidatingNotaryFlow.kt:24-52
    checkSignatures: stx.verifySignatures(notaryKey), SignaturesMissingException -> SignaturesMissing;
    SignatureException -> TransactionInvalid; anything else (IllegalStateException, InvalidKeyException)
    is re-thrown: the flow fails
  commitInputStates                      NotaryFlow.kt:133-141
    UniquenessException -> Conflict(tx, SignedData(serialized conflict, notary signature over it))
  TimestampChecker.isValid               core/.../node/services/TimestampChecker.kt:13-26

`BatchingNotary.notarise(requests)` runs that decision procedure for a whole batch: ONE Merkle call
recomputes every tx id (an empty transaction fails only its own request), ONE verify call checks
every signature of every transaction — sharded over the ranks of a process group when one is given,
each rank verifying its 64-aligned slice on its own GPU and ONE all-gather (RCCL under the "nccl"
backend) replicating the verdict and key-status bitmaps into the commit step — then inputs are
committed in request order (so conflicts resolve exactly as sequential flows would) and the notary
signs every accepted id and every conflict report in ONE GPU signing call.  Contract verification is
out of scope; dependency resolution (ResolveTransactionsFlow) is corda_amd.resolve's
(DESIGN.md §5.13), not this mirror's.

A request that the reference answers with a Result carries `error` (a NotaryError); one whose flow
the reference fails by an exception carries `failure` (that exception) instead — the client sees
the flow end with it, never a notary signature.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from . import native
from .crypto import (CompositeKey, DigitalSignature, EdDSAPublicKey, IllegalArgumentException, IllegalStateException,
                     InvalidKeyException, KeyPair, SignatureException, VerifyItem, _prefilter, verify_many,
                     verify_with_ecdsa)
from .transactions import (MerkleTreeException, SecureHash, SignaturesMissingException, SignedTransaction,
                           WireTransaction, _device_decidable, _missing_exception, compute_ids, flatten_must_sign,
                           flatten_signatures, missing_signatures_batch, must_sign_reqs)


# ---------------------------------------------------------------- timestamps (Structures.kt:412-423)
@dataclass(frozen=True)
class Timestamp:
    """Timestamp(after, before) in epoch seconds; at least one bound, after <= before."""
    after: Optional[float]
    before: Optional[float]

    def __post_init__(self):
        if self.after is None and self.before is None:
            raise IllegalArgumentException("At least one of before/after must be specified")
        if self.after is not None and self.before is not None and not self.after <= self.before:
            raise IllegalStateException("Check failed.")

    @staticmethod
    def around(time_s: float, tolerance_s: float) -> "Timestamp":
        return Timestamp(time_s - tolerance_s, time_s + tolerance_s)


class TimestampChecker:
    """TimestampChecker.kt:13-26: valid iff neither bound is further than `tolerance` from now."""

    def __init__(self, clock: Callable[[], float] = time.time, tolerance: float = 30.0):
        self.clock = clock
        self.tolerance = tolerance

    def is_valid(self, ts: Timestamp) -> bool:
        now = self.clock()
        if ts.before is not None and now - ts.before > self.tolerance:
            return False
        if ts.after is not None and ts.after - now > self.tolerance:
            return False
        return True


# ---------------------------------------------------------------- uniqueness (corda_amd/uniqueness.py)
from .uniqueness import (ConsumingTx, InMemoryUniquenessProvider, PersistentUniquenessProvider,  # noqa: E402,F401
                         UniquenessConflict, UniquenessException)


@dataclass
class SignedData:
    """SignedData.kt:14-39: serialized bytes + a signature over them; verified() checks the signature
    (SignatureException when it does not match) and returns the deserialized conflict."""
    raw: bytes
    sig: DigitalSignature.WithKey

    def verified(self, engine: Optional[native.Engine] = None) -> UniquenessConflict:
        verify_with_ecdsa(self.sig.by, self.raw, self.sig, engine)
        return UniquenessConflict.deserialize(self.raw)


# ---------------------------------------------------------------- NotaryError (NotaryFlow.kt:163-176)
class NotaryError:
    pass


@dataclass
class Conflict(NotaryError):
    tx: WireTransaction
    conflict: SignedData

    def __str__(self):
        return f"One or more input states for transaction {self.tx.id!r} have been used in another transaction"


@dataclass
class TimestampInvalid(NotaryError):
    pass


@dataclass
class TransactionInvalid(NotaryError):
    pass


@dataclass
class SignaturesMissing(NotaryError):
    missing_signers: set


class NotaryException(Exception):
    def __init__(self, error: NotaryError):
        super().__init__(f"Error response from Notary - {error}")
        self.error = error


# ---------------------------------------------------------------- requests and results
@dataclass
class SignRequest:
    stx: SignedTransaction
    caller: str
    input_refs: Optional[List[object]] = None     # StateRefs; default: the serialized input leaves
    timestamp: Optional[Timestamp] = None         # wtx.timestamp (the mirror's leaves are not decoded)


@dataclass
class Result:
    """Result.Success(sig) (ok), Result.Error(error), or the flow's failure exception (failure)."""
    ok: bool
    sig: Optional[DigitalSignature.WithKey] = None
    error: Optional[NotaryError] = None
    failure: Optional[Exception] = None

    def get_or_throw(self) -> DigitalSignature.WithKey:
        """What NotaryFlow.Client returns or throws (NotaryFlow.kt:56-72)."""
        if self.failure is not None:
            raise self.failure
        if self.error is not None:
            raise NotaryException(self.error)
        return self.sig


# ---------------------------------------------------------------- verification, sharded over ranks
def verify_many_sharded(items: Sequence[VerifyItem], engine, group=None) -> List[Optional[Exception]]:
    """verify_many over a process group: rank r verifies its 64-aligned slice of the items on its own
    engine; the verdict bits and the bad-key bits of every slice are replicated to every rank by ONE
    all-gather (distributed.gather_bitmaps; RCCL under "nccl", CPU tensors under "gloo"); every
    rank then rebuilds the same per-item exceptions verify_many returns for the whole list."""
    import torch
    import torch.distributed as dist
    from . import distributed as D

    n = len(items)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    b, e = D.shard_range(n, world, rank)
    per = D.shard_words(n, world)
    errs = verify_many(items[b:e], engine) if e > b else []
    ok = np.zeros(per * 64, bool)
    bad_key = np.zeros(per * 64, bool)
    for j, err in enumerate(errs):
        ok[j] = err is None
        bad_key[j] = isinstance(err, InvalidKeyException)
    local = np.stack([np.packbits(ok, bitorder="little").view("<i8"), np.packbits(bad_key, bitorder="little").view("<i8")])
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    glob = D.gather_bitmaps(torch.from_numpy(local).to(dev), n, group).cpu().numpy().view(np.uint64)
    okg = native.bitmap_to_bools(glob[0], n)
    badg = native.bitmap_to_bools(glob[1], n)
    out: List[Optional[Exception]] = []
    for i, it in enumerate(items):
        if okg[i]:
            out.append(None)
            continue
        pre = _prefilter(it)
        out.append(pre if pre is not None else
                   InvalidKeyException("not a valid GroupElement") if badg[i] else
                   SignatureException("Signature did not match"))
    return out


# ---------------------------------------------------------------- the notary
class BatchingNotary:
    def __init__(self, notary_seed: bytes, validating: bool = True, engine: Optional[native.Engine] = None,
                 uniqueness=None,
                 timestamp_checker: Optional[TimestampChecker] = None, group=None, device_signers: bool = False,
                 fused: bool = False):
        """fused=True: notarise() makes ONE cv_notarise_batch call per batch (ids, signatures, missing signers, the
        commit and the notary's signatures on the device, the reference's precedence settled in the library) and one
        further signing call for the conflict reports.  It needs a DeviceUniquenessProvider(leaf_keys=True) and no
        process group.  In fused mode a request with explicit input_refs, or with a mustSign entry the device cannot
        decide (transactions._device_decidable: a Leaf that is not a 32-byte EdDSA key, weights outside Int), raises
        IllegalArgumentException: the states are the input leaves and every requirement is decided on the device."""
        self.engine = engine or native.default_engine()
        self.fused = fused
        # the missing signers of a whole batch in one device call (transactions.missing_signatures_batch) instead of
        # one host evaluation per request; off by default, as the device uniqueness provider is
        self.device_signers = device_signers
        # the notary's one long-lived key, expanded once on the engine's devices (cv_signer)
        self.key_pair = KeyPair(bytes(notary_seed), self.engine)
        self.public_key: EdDSAPublicKey = self.key_pair.public
        self.owning_key: CompositeKey = self.public_key.composite
        self.validating = validating
        self.uniqueness = uniqueness if uniqueness is not None else InMemoryUniquenessProvider()
        self.timestamp_checker = timestamp_checker or TimestampChecker()
        self.group = group
        if fused and (group is not None or not getattr(self.uniqueness, "leaf_keys", False)):
            raise IllegalArgumentException("fused=True needs a DeviceUniquenessProvider(leaf_keys=True) and no process group")

    def _verify(self, items: List[VerifyItem]) -> List[Optional[Exception]]:
        if self.group is not None:
            return verify_many_sharded(items, self.engine, self.group)
        return verify_many(items, self.engine)

    def _sign(self, msgs: List[bytes]) -> List[DigitalSignature.WithKey]:
        """The notary key over every message, in one GPU signing call (the fixed-key signer)."""
        return self.key_pair.sign_many(msgs)

    def _notarise_fused(self, requests: Sequence[SignRequest]) -> List[Result]:
        """notarise() through cv_notarise_batch: the batch flattened once, keys and lengths prefiltered into sig_pre,
        TimestampChecker into tx_pre, one call, then the same Result objects as the unfused path."""
        n = len(requests)
        for r in requests:
            if r.input_refs is not None:
                raise IllegalArgumentException("fused notary: the states are the transaction's input leaves (input_refs given)")
            if self.validating and not all(_device_decidable(k) for k in r.stx._wtx.must_sign):
                raise IllegalArgumentException("fused notary: a mustSign entry that the device cannot decide")
        leaves: List[bytes] = []
        txb, nin = [0], []
        for r in requests:
            leaves.extend(r.stx._wtx.leaves)
            txb.append(len(leaves))
            nin.append(len(r.stx._wtx.inputs))
        arena, offs, lens = native.pack_blobs(leaves)
        claimed = np.frombuffer(b"".join(r.stx.id.bytes for r in requests), np.uint8)
        tx_pre = np.array([1 if r.timestamp is not None and not self.timestamp_checker.is_valid(r.timestamp) else 0
                           for r in requests], np.uint8)
        sigs = reqs = None
        pre_err: Dict[int, Exception] = {}
        if self.validating:
            stxs = [r.stx for r in requests]
            sigs, keys, pre_err = flatten_signatures(stxs)
            reqs = must_sign_reqs(flatten_must_sign(stxs, (self.owning_key,)), keys, allowed=True)

        def call(uniq, handles):
            out = self.engine.notarise_batch(uniq, self.key_pair._signer, arena, offs, lens, np.array(txb, np.uint32),
                                             np.array(nin, np.uint32), claimed, handles, tx_pre, sigs=sigs, reqs=reqs)
            rows = [(state, requests[k].stx.id.bytes, i, requests[k].caller)
                    for k in np.flatnonzero(out["outcome"] == native.CV_NS_SUCCESS)
                    for i, state in enumerate(requests[k].stx._wtx.inputs)]
            return out, rows                   # the provider appends the rows to its log before any signature is released

        out, parties = self.uniqueness.fused([r.caller for r in requests], int(sum(nin)), call)
        outcome = out["outcome"]
        if (outcome == native.CV_NS_MALFORMED).any():
            raise IllegalStateException("cv_notarise_batch: the flattened mustSign trees came back malformed")
        results: List[Optional[Result]] = [None] * n
        conflicts: List[tuple] = []
        sbeg = np.concatenate([[0], np.cumsum(nin)])
        for k, r in enumerate(requests):
            o, w = int(outcome[k]), r.stx._wtx
            if o != native.CV_NS_EMPTY and w._id is None:
                w._id = SecureHash(out["ids"][k].tobytes())
            if o == native.CV_NS_SUCCESS:
                results[k] = Result(True, sig=DigitalSignature.WithKey(self.public_key, out["notary_sig"][k].tobytes()))
            elif o == native.CV_NS_EMPTY:
                results[k] = Result(False, failure=MerkleTreeException("Cannot calculate Merkle root on empty hash list."))
            elif o == native.CV_NS_ID_MISMATCH:
                try:
                    r.stx.tx
                    raise IllegalStateException("cv_notarise_batch: an id mismatch the mirror does not see")
                except IllegalStateException as e:
                    results[k] = Result(False, failure=e)
            elif o == native.CV_NS_TIMESTAMP_INVALID:
                results[k] = Result(False, error=TimestampInvalid())
            elif o == native.CV_NS_TX_INVALID:
                results[k] = Result(False, error=TransactionInvalid())
            elif o == native.CV_NS_BAD_KEY:
                i = int(out["first_bad"][k])
                results[k] = Result(False, failure=pre_err.get(i) or InvalidKeyException("not a valid GroupElement"))
            elif o == native.CV_NS_SIGNATURES_MISSING:
                b, e = int(reqs[7][k]), int(reqs[7][k + 1])
                need = {w.must_sign[i] for i in range(e - b) if out["req_missing"][b + i] == 1 and not reqs[9][b + i]}
                results[k] = Result(False, error=SignaturesMissing(_missing_exception(r.stx, need).missing))
            else:                                                  # CV_NS_CONFLICT
                b = int(sbeg[k])
                c = UniquenessConflict({s: ConsumingTx(SecureHash(out["consumed_id"][b + j].tobytes()),
                                                       int(out["consumed_index"][b + j]),
                                                       parties[int(out["consumed_caller"][b + j])])
                                        for j, s in enumerate(w.inputs) if out["state_conflict"][b + j]})
                conflicts.append((k, c.serialize()))
        csigs = self._sign([raw for _, raw in conflicts]) if conflicts else []
        for (k, raw), sig in zip(conflicts, csigs):
            results[k] = Result(False, error=Conflict(requests[k].stx.tx, SignedData(raw, sig)))
        return results  # type: ignore[return-value]

    def notarise(self, requests: Sequence[SignRequest]) -> List[Result]:
        n = len(requests)
        if self.fused:
            return self._notarise_fused(requests) if n else []
        results: List[Optional[Result]] = [None] * n
        # val wtx = stx.tx: every unknown id in one Merkle call, then check(temp.id == id) per request
        unknown = [r.stx._wtx for r in requests if r.stx._wtx._id is None]
        if unknown:
            compute_ids(unknown, self.engine)
        failed: List[Optional[Exception]] = [None] * n
        for k, r in enumerate(requests):
            try:
                r.stx.tx
            except (IllegalStateException, MerkleTreeException) as e:
                failed[k] = e
        # the signatures of every transaction in one verify call (validating notary only)
        first_bad: List[Optional[Exception]] = [None] * n
        if self.validating:
            items, begin = [], [0]
            for k, r in enumerate(requests):
                if failed[k] is None:
                    items.extend(VerifyItem(s.by, r.stx.id.bytes, s.bits) for s in r.stx.sigs)
                begin.append(len(items))
            errs = self._verify(items)
            for k in range(n):
                first_bad[k] = next((e for e in errs[begin[k]:begin[k + 1]] if e is not None), None)
        missing: Dict[int, Optional[Exception]] = {}
        if self.validating and self.device_signers:
            ks = [k for k in range(n) if failed[k] is None and first_bad[k] is None]
            missing = dict(zip(ks, missing_signatures_batch([requests[k].stx for k in ks], (self.owning_key,),
                                                            self.engine)))
        accepted: List[int] = []
        conflicts: List[tuple] = []
        to_commit: List[tuple] = []
        for k, r in enumerate(requests):
            if failed[k] is not None:
                results[k] = Result(False, failure=failed[k])
                continue
            if r.timestamp is not None and not self.timestamp_checker.is_valid(r.timestamp):
                results[k] = Result(False, error=TimestampInvalid())
                continue
            if self.validating:
                e = first_bad[k]
                if e is None and self.device_signers:
                    if missing[k] is not None:
                        results[k] = Result(False, error=SignaturesMissing(missing[k].missing))
                        continue
                elif e is None:
                    try:
                        r.stx._finish_verify((self.owning_key,))
                    except SignaturesMissingException as ex:
                        results[k] = Result(False, error=SignaturesMissing(ex.missing))
                        continue
                    except Exception as ex:  # noqa: BLE001 - mirrored reference exceptions
                        e = ex
                if e is not None:
                    if isinstance(e, SignatureException):
                        results[k] = Result(False, error=TransactionInvalid())
                    else:                                      # ValidatingNotaryFlow.kt:35: else -> throw e
                        results[k] = Result(False, failure=e)
                    continue
            refs = r.input_refs if r.input_refs is not None else list(r.stx._wtx.inputs)
            to_commit.append((k, refs))
        # commitInputStates for the whole batch, decided in request order (uniqueness.py)
        reqs = [(refs, requests[k].stx.id, requests[k].caller) for k, refs in to_commit]
        if hasattr(self.uniqueness, "commit_batch"):
            decided = self.uniqueness.commit_batch(reqs)
        else:
            decided = []
            for states, tx_id, caller in reqs:
                try:
                    self.uniqueness.commit(states, tx_id, caller)
                    decided.append(None)
                except UniquenessException as ex:
                    decided.append(ex.error)
        for (k, _), c in zip(to_commit, decided):
            if c is None:
                accepted.append(k)
            else:
                conflicts.append((k, c.serialize()))
        msgs = [requests[k].stx.id.bytes for k in accepted] + [raw for _, raw in conflicts]
        sigs = self._sign(msgs) if msgs else []
        for j, k in enumerate(accepted):
            results[k] = Result(True, sig=sigs[j])
        for j, (k, raw) in enumerate(conflicts):
            results[k] = Result(False, error=Conflict(requests[k].stx.tx, SignedData(raw, sigs[len(accepted) + j])))
        return results  # type: ignore[return-value]
