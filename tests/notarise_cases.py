"""Cases and the reference restatement for cv_notarise_batch, shared by tests/test_notary_cpu.py (the lane functions of
corda_amd/csrc/cv_notary.h on the CPU) and tests/test_gpu_notarise.py (the entry point on the GPU).  Pure Python.

The restatement is NotaryFlow.Service.call (NotaryFlow.kt:96-146) with ValidatingNotaryFlow.beforeCommit
(ValidatingNotaryFlow.kt:24-45) over plain data, written as the reference's control flow: exceptions thrown where the
reference throws them and caught where it catches them.  A transaction is a dict:
    mstatus    0, or 1 = no leaves (MerkleTreeException out of WireTransaction.id)
    claimed, recomputed   32 bytes each (SignedTransaction.id and the id of its leaves)
    tx_pre     non-zero = TimestampChecker.isValid said no
    sigs       [(verdict bit, device status CV_SIG_*, sig_pre 0/1/2)] in the order of stx.sigs
    ck         the missing-signers status CV_VS_* (verifySignatures' verdict after the signature checks)
    states     [32-byte keys] of its inputs, caller the requesting party's handle
"""
import hashlib

import numpy as np

SUCCESS, EMPTY, ID_MISMATCH, TIMESTAMP_INVALID, TX_INVALID, BAD_KEY, SIGNATURES_MISSING, MALFORMED, CONFLICT = range(9)
NO_SIG = 0xFFFFFFFF
VS_OK, VS_BAD_SIGNATURE, VS_MISSING, VS_MALFORMED = 0, 1, 2, 3
SIG_BAD_KEY = 1
PRE_SIGNATURE, PRE_KEY = 1, 2
UNIQ_OK, UNIQ_CONFLICT, UNIQ_SKIPPED = 0, 1, 2


# ---------------------------------------------------------------- the reference, restated
class MerkleTreeException(Exception):
    pass


class IllegalStateException(Exception):
    pass


class SignatureException(Exception):
    pass


class InvalidKeyException(Exception):
    pass


class SignaturesMissingException(SignatureException):     # SignedTransaction.kt:47: it IS a SignatureException
    pass


class MalformedRequirement(Exception):                    # CV_VS_MALFORMED has no reference counterpart
    pass


class NotaryException(Exception):
    def __init__(self, error):
        super().__init__(error)
        self.error = error


class UniquenessException(Exception):
    def __init__(self, conflict):
        super().__init__("conflict")
        self.conflict = conflict


class SequentialProvider:
    """InMemoryUniquenessProvider.kt:14-36 over a dict: key -> (tx id, input index, caller)."""

    def __init__(self, resident=None):
        self.committed = dict(resident or {})

    def commit(self, states, tx_id, caller):
        conflict = {k: self.committed[k] for k in states if k in self.committed}
        if conflict:
            raise UniquenessException(conflict)
        for j, k in enumerate(states):
            self.committed[k] = (tx_id, j, caller)


def _tx(tx):
    """val wtx = stx.tx (SignedTransaction.kt:34-38): the id of the leaves, checked against the claimed one."""
    if tx["mstatus"]:
        raise MerkleTreeException("Cannot calculate Merkle root on empty hash list.")
    if tx["recomputed"] != tx["claimed"]:
        raise IllegalStateException("Supplied transaction ID does not match deserialized transaction's ID")


def _check_signatures_are_valid(tx, note):
    """SignedTransaction.kt:82-87: for (sig in sigs) sig.verifyWithECDSA(id.bytes) — the first failure throws."""
    for i, (bit, status, pre) in enumerate(tx["sigs"]):
        if pre == PRE_KEY:
            note["first_bad"] = i
            raise InvalidKeyException("not an EdDSA key")
        if pre:
            note["first_bad"] = i
            raise SignatureException("signature length is wrong")
        if not bit:
            note["first_bad"] = i
            if status == SIG_BAD_KEY:
                raise InvalidKeyException("not a valid GroupElement")
            raise SignatureException("Signature did not match")


def _verify_signatures(tx, note):
    """SignedTransaction.kt:58-72 (sigs.isNotEmpty() is the constructor's rule, cv_tx_verdicts')."""
    if not tx["sigs"]:
        raise SignatureException("no signatures")
    _check_signatures_are_valid(tx, note)
    if tx["ck"] == VS_MALFORMED:
        raise MalformedRequirement()
    if tx["ck"] == VS_MISSING:
        raise SignaturesMissingException("missing")


def _before_commit(tx, validating, note):
    """ValidatingNotaryFlow.kt:24-45; NotaryFlow.kt:129-131 when not validating."""
    if not validating:
        return
    try:
        try:
            _verify_signatures(tx, note)
        except SignaturesMissingException:
            raise NotaryException(SIGNATURES_MISSING)
    except SignatureException:
        raise NotaryException(TX_INVALID)


def service_call(tx, validating, commit):
    """NotaryFlow.kt:96-113 for one request -> (outcome, first_bad relative to the transaction or None, conflict).
    commit(tx) is commitInputStates' uniquenessProvider.commit: it raises UniquenessException."""
    note = {"first_bad": None}
    try:
        _tx(tx)                                   # outside the try: the flow fails
    except MerkleTreeException:
        return EMPTY, None, None
    except IllegalStateException:
        return ID_MISMATCH, None, None
    try:
        if tx["tx_pre"]:
            raise NotaryException(TIMESTAMP_INVALID)
        _before_commit(tx, validating, note)
        try:
            commit(tx)
        except UniquenessException as e:
            note["conflict"] = e.conflict
            raise NotaryException(CONFLICT)
        return SUCCESS, None, None
    except NotaryException as e:
        return e.error, note["first_bad"], note.get("conflict")
    except InvalidKeyException:                   # ValidatingNotaryFlow.kt:34 else -> throw e: the flow fails
        return BAD_KEY, note["first_bad"], None
    except MalformedRequirement:
        return MALFORMED, None, None


def gate(txs, validating):
    """The outcome before the commit of every transaction -> (pre u8, enable u8, first_bad u32 absolute)."""
    pre, fb, base = [], [], 0
    for tx in txs:
        out, bad, _ = service_call(tx, validating, lambda _tx: None)
        pre.append(out)
        fb.append(NO_SIG if bad is None else base + bad)
        base += len(tx["sigs"]) if validating else 0
    pre = np.array(pre, np.uint8)
    return pre, (pre == SUCCESS).astype(np.uint8), np.array(fb, np.uint32)


def notarise(txs, validating, resident=None):
    """The whole batch, one request after another on one provider -> dict of the expected outputs."""
    prov = SequentialProvider(resident)
    outcome, fb, sc, cid, cix, cc, base = [], [], [], [], [], [], 0
    for tx in txs:
        out, bad, conflict = service_call(tx, validating, lambda x: prov.commit(x["states"], x["recomputed"], x["caller"]))
        outcome.append(out)
        fb.append(NO_SIG if bad is None else base + bad)
        base += len(tx["sigs"]) if validating else 0
        for k in tx["states"]:
            rec = (conflict or {}).get(k)
            sc.append(1 if rec else 0)
            cid.append(np.frombuffer(rec[0] if rec else bytes(32), np.uint8))
            cix.append(rec[1] if rec else 0)
            cc.append(rec[2] if rec else 0)
    outcome = np.array(outcome, np.uint8)
    return dict(outcome=outcome, first_bad=np.array(fb, np.uint32), accepted=np.flatnonzero(outcome == SUCCESS).astype(np.uint32),
                state_conflict=np.array(sc, np.uint8), consumed_id=np.array(cid, np.uint8).reshape(-1, 32),
                consumed_index=np.array(cix, np.uint32), consumed_caller=np.array(cc, np.uint32), committed=prov.committed)


# ---------------------------------------------------------------- plain cases
def h32(*parts) -> bytes:
    return hashlib.sha256(repr(parts).encode()).digest()


def make_tx(tag, states=(), sigs=((1, 0, 0),), **kw):
    tx = dict(mstatus=0, recomputed=h32("id", tag), tx_pre=0, sigs=list(sigs), ck=VS_OK, states=list(states), caller=7)
    tx["claimed"] = tx["recomputed"]
    tx.update(kw)
    if tx["mstatus"]:
        tx["recomputed"] = bytes(32)
    return tx


def _ck_of(sigs, missing, malformed):
    """cv_missing_signers' tx_status for these conditions (its own precedence: malformed, bad signature, missing)."""
    if malformed:
        return VS_MALFORMED
    if not sigs or any(not s[0] for s in sigs):
        return VS_BAD_SIGNATURE
    return VS_MISSING if missing else VS_OK


def precedence_cases():
    """Every combination of the seven gating conditions on one transaction (empty, id mismatch, timestamp, a bad
    signature, a bad key, a missing signer, a malformed requirement), the bad key before and after the bad signature,
    each with one fresh input state."""
    txs = []
    for m in range(128):
        empty, mism, ts, badsig, badkey, missing, malformed = [(m >> b) & 1 for b in range(7)]
        for key_first in ((0, 1) if badsig and badkey else (0,)):
            bad = [(0, 0, 0)] * badsig + [(0, SIG_BAD_KEY, 0)] * badkey
            sigs = [(1, 0, 0)] + (bad[::-1] if key_first else bad) + [(1, 0, 0)]
            tx = make_tx(("prec", m, key_first), [h32("prec-state", m, key_first)], sigs, mstatus=empty, tx_pre=ts,
                         ck=_ck_of(sigs, missing, malformed))
            if mism:
                tx["claimed"] = h32("other", m)
            txs.append(tx)
    return txs


def prefilter_cases():
    """sig_pre decides before the verdict bit and the device status do; a transaction without signatures."""
    a = h32("pre-state")
    return [make_tx("p0", [a], [(1, 0, PRE_SIGNATURE)], ck=VS_OK),
            make_tx("p1", [a], [(1, 0, 0), (0, SIG_BAD_KEY, PRE_SIGNATURE)], ck=VS_BAD_SIGNATURE),
            make_tx("p2", [a], [(0, 0, PRE_KEY), (0, 0, 0)], ck=VS_BAD_SIGNATURE),
            make_tx("p3", [a], [(1, SIG_BAD_KEY, 0)]),                    # a set bit wins over the status byte
            make_tx("p4", [a], []),
            make_tx("p5", [a], [(1, 0, 0)] * 70 + [(0, 0, 0)], ck=VS_BAD_SIGNATURE),   # past a bitmap word
            make_tx("p6", [a])]


def neighbour_cases():
    """A batch whose neighbours hit different outcomes, 1-3 signatures each so that ranges straddle bitmap words."""
    txs = []
    for t in range(150):
        kind = t % 9
        nsig = 1 + t % 3
        sigs = [(1, 0, 0)] * nsig
        kw = {}
        if kind == EMPTY:
            kw["mstatus"] = 1
        elif kind == TIMESTAMP_INVALID:
            kw["tx_pre"] = 1
        elif kind == TX_INVALID:
            sigs[-1] = (0, 0, 0)
        elif kind == BAD_KEY:
            sigs[0] = (0, SIG_BAD_KEY, 0)
        elif kind == SIGNATURES_MISSING:
            kw["ck"] = VS_MISSING
        elif kind == MALFORMED:
            kw["ck"] = VS_MALFORMED
        if kind in (TX_INVALID, BAD_KEY):
            kw["ck"] = VS_BAD_SIGNATURE
        # CONFLICT: the state of the accepted transaction nine before it
        states = [h32("nb", t - 8 if kind == CONFLICT else t)] + [h32("nb2", t, j) for j in range(t % 3)]
        tx = make_tx(("nb", t), states, sigs, caller=t % 5, **kw)
        if kind == ID_MISMATCH:
            tx["claimed"] = h32("nb-other", t)
        txs.append(tx)
    return txs


def conflict_cases():
    """Conflicts with an earlier accepted request, none with an earlier rejected one, resident states, chains, requests
    without inputs and with repeated inputs."""
    s = [h32("cs", i) for i in range(40)]
    txs = [make_tx("c0", [s[0], s[1]]),
           make_tx("c1", [s[1], s[2]]),                       # conflicts with c0 on s1
           make_tx("c2", [s[2], s[3]]),                       # c1 was rejected: s2 is free
           make_tx("c3", [s[4]], tx_pre=1),                   # gated out: commits nothing
           make_tx("c4", [s[4]]),                             # so this one is accepted
           make_tx("c5", [s[30]]),                            # resident
           make_tx("c6", [s[5], s[31], s[6]]),                # one resident among fresh ones
           make_tx("c7", []),                                 # no inputs: accepted
           make_tx("c8", [s[7], s[7], s[8], s[7]]),           # repeated input: the last index wins
           make_tx("c9", [s[7]]),                             # conflicts with c8, index 3
           make_tx("c10", [s[6]])]                            # c6 was rejected: s6 is free
    txs += [make_tx(("chain", t), [s[10 + t], s[11 + t]], caller=t) for t in range(12)]   # every other one is accepted
    resident = {s[30]: (h32("old", 0), 2, 3), s[31]: (h32("old", 1), 0, 4)}
    return txs, resident


CASES = {"precedence": lambda: (precedence_cases(), {}), "prefilter": lambda: (prefilter_cases(), {}),
         "neighbours": lambda: (neighbour_cases(), {}), "conflicts": conflict_cases}


def flatten(txs, validating=True):
    """The plain cases as the arrays the gate and finalise lanes read."""
    n = len(txs)
    tsb = np.zeros(n + 1, np.uint32)
    bits, status, pre = [], [], []
    for t, tx in enumerate(txs):
        for b, s, p in (tx["sigs"] if validating else ()):
            bits.append(b), status.append(s), pre.append(p)
        tsb[t + 1] = len(bits)
    bm = np.zeros(max((len(bits) + 63) // 64, 1), np.uint64)
    for i, b in enumerate(bits):
        if b:
            bm[i // 64] |= np.uint64(1) << np.uint64(i % 64)
    sbeg = np.concatenate([[0], np.cumsum([len(tx["states"]) for tx in txs])]).astype(np.uint32)
    keys = [k for tx in txs for k in tx["states"]]
    return dict(ntx=n, mstatus=np.array([tx["mstatus"] for tx in txs], np.uint8),
                id=np.frombuffer(b"".join(tx["recomputed"] for tx in txs), np.uint8).reshape(n, 32).copy(),
                claimed=np.frombuffer(b"".join(tx["claimed"] for tx in txs), np.uint8).reshape(n, 32).copy(),
                tx_pre=np.array([tx["tx_pre"] for tx in txs], np.uint8), tx_sig_begin=tsb, bitmap=bm,
                sig_status=np.array(status + [0], np.uint8), sig_pre=np.array(pre + [0], np.uint8),
                ck=np.array([tx["ck"] for tx in txs], np.uint8), caller=np.array([tx["caller"] for tx in txs], np.uint32),
                state_begin=sbeg, key=np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32).copy() if keys
                else np.zeros((0, 32), np.uint8))
