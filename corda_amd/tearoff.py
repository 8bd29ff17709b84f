"""The tear-off oracle: NodeInterestRates.Oracle (samples/irs-demo/src/main/kotlin/net/corda/irs/api/
NodeInterestRates.kt:190-225; its client is RatesFixFlow.kt:100-110) for a batch of signing requests.

    oracle = TearOffOracle(key_pair, classify)
    results = oracle.sign_batch([(ftx, merkle_root), ...])

sign_batch makes ONE cv_tearoff_sign_batch call: the filtered leaves hashed on the device, the partial trees verified
against the roots, the oracle's refusals settled in the reference's order, the accepted roots signed with the
oracle's fixed key.  What stays with the binding is the content of the leaves — the Kryo decode and
the table of known fixes — behind `classify`.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Union

from . import native
from .crypto import DigitalSignature, IllegalArgumentException, KeyPair
from .transactions import MerkleTreeException, flatten_filtered


class UnknownFix(Exception):
    """NodeInterestRates.UnknownFix (a RetryableException): `leaf` is the index, among the tear-off's filtered
    leaves, of the first fix the oracle does not know as given; `leaf_bytes` its serialised command."""

    def __init__(self, leaf: int, leaf_bytes: bytes):
        super().__init__(f"Unknown fix: filtered leaf {leaf}")
        self.leaf, self.leaf_bytes = leaf, leaf_bytes


class TearOffOracle:
    """NodeInterestRates.Oracle's signing half.  signer: the oracle's KeyPair (or a native.Signer).
    classify(group, leaf_bytes) -> 0..3 stands in for the Kryo decode and the fix table, group being "inputs",
    "outputs", "attachments" or "commands": native.TS_PRE_OK; TS_PRE_NOT_COMMAND — an input, output or attachment
    (classify says so itself: the group is passed for that); TS_PRE_WRONG_COMMAND — not a Fix, or the oracle is not
    among its signers; TS_PRE_UNKNOWN — a fix the oracle does not know, or knows differently."""

    def __init__(self, signer: Union[KeyPair, native.Signer], classify: Callable[[str, bytes], int],
                 engine: Optional[native.Engine] = None):
        self.key_pair = signer if isinstance(signer, KeyPair) else None
        self._signer = signer._signer if isinstance(signer, KeyPair) else signer
        self.classify = classify
        self.engine = engine or self._signer._engine

    def sign_batch(self, items: Sequence) -> List[Union[DigitalSignature.WithKey, bytes, Exception]]:
        """items: (ftx, merkle_root).  Per item the signature — a DigitalSignature.WithKey when the oracle was built
        on a KeyPair, else the 64 bytes — or the exception the sequential reference would throw for it:
        MerkleTreeException (no filtered leaves; the tree does not verify), IllegalArgumentException (the nodes are no
        tree; something other than commands; a command the oracle does not vouch for) or UnknownFix."""
        if not items:
            return []
        args = flatten_filtered(items, self.classify)
        outcome, first_bad, sig = self.engine.tearoff_sign_batch(self._signer, *args)
        txb = args[3]
        res: list = []
        for t, (ftx, _) in enumerate(items):
            o = int(outcome[t])
            if o == native.CV_TS_SUCCESS:
                bits = sig[t].tobytes()
                res.append(DigitalSignature.WithKey(self.key_pair.public, bits) if self.key_pair else bits)
            elif o == native.CV_TS_NO_LEAVES:
                res.append(MerkleTreeException("Transaction without included leaves."))
            elif o == native.CV_TS_MALFORMED:
                res.append(IllegalArgumentException("malformed partial Merkle tree encoding"))
            elif o == native.CV_TS_VERIFY_FAILED:
                res.append(MerkleTreeException("Rate Fix Oracle: Couldn't verify partial Merkle tree."))
            elif o == native.CV_TS_UNKNOWN:
                k = int(first_bad[t]) - int(txb[t])
                fl = ftx.filtered_leaves
                res.append(UnknownFix(k, (fl.inputs + fl.outputs + fl.attachments + fl.commands)[k]))
            else:
                res.append(IllegalArgumentException("Failed requirement." if o == native.CV_TS_NOT_COMMANDS else
                                                    "more commands than the oracle signs"))
        return res
