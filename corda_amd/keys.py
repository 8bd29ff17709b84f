"""Host-side mirror of the node's key management service and of the builder's signing step, backed by the device key
store (native.KeyStore).

Mirrors:
  KeyManagementService (keys, toPrivate, freshKey)   core/src/main/kotlin/net/corda/core/node/services/Services.kt:206-219
  PersistentKeyManagementService / E2ETestKeyManagementService
                                                     node/src/main/kotlin/net/corda/node/services/keys/
                                                     PersistentKeyManagementService.kt:40-66
  TransactionBuilder.signWith / toSignedTransaction  core/src/main/kotlin/net/corda/core/transactions/TransactionBuilder.kt:93-98,132-141
  the flows' signing loops                           finance/.../flows/CashFlow.kt:39-47, TwoPartyTradeFlow.kt:227-235,250

The reference's freshKey() returns a KeyPair and `keys` maps to PrivateKey objects; here the private halves never leave
the service — fresh_key() returns the public key, `keys` is the set of public halves, and signing is a method of the
service (sign, sign_many), as the interface's own comment says a real one would be.  Seeds are the caller's: a node
keeps them durable (PersistentKeyManagementService's table) and hands them back as initial_seeds after a restart.
"""
from __future__ import annotations

import os
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import native
from .crypto import DigitalSignature, EdDSAPublicKey, IllegalStateException, KeyPair, OpaqueBytes, PublicKey
from .transactions import (MerkleTreeException, SecureHash, SignedTransaction, WireTransaction, compute_ids,
                           missing_signatures_batch)


def _no_key(public_key: PublicKey) -> IllegalStateException:
    return IllegalStateException(f"No private key known for requested public key {public_key!r}")   # Services.kt:210


def _content(content) -> bytes:
    if isinstance(content, OpaqueBytes):
        return content.bits
    return content.bytes if isinstance(content, SecureHash) else bytes(content)


def _entropy(n: int, entropy) -> np.ndarray:
    raw = os.urandom(32 * n) if entropy is None else bytes(entropy)
    if len(raw) != 32 * n:
        raise ValueError(f"entropy must be {32 * n} bytes, 32 per key")
    return np.frombuffer(raw, np.uint8).reshape(n, 32)


class InMemoryKeyManagementService:
    """E2ETestKeyManagementService: a dict PublicKey -> crypto.KeyPair, one fixed-key signer per key.  The composed path:
    what a node had before the device store, and what the tests compare DeviceKeyManagementService with."""

    def __init__(self, engine: Optional[native.Engine] = None, initial_seeds: Iterable[bytes] = ()):
        self.engine = engine or native.default_engine()
        self._pairs = {}
        for seed in initial_seeds:
            self._put(bytes(seed))

    def _put(self, seed: bytes) -> EdDSAPublicKey:
        kp = KeyPair(seed, self.engine)
        if kp.public in self._pairs:
            kp.close()
        else:
            self._pairs[kp.public] = kp
        return kp.public

    def close(self) -> None:
        for kp in self._pairs.values():
            kp.close()
        self._pairs = {}

    def fresh_keys(self, n: int, entropy=None) -> List[EdDSAPublicKey]:
        return [self._put(row.tobytes()) for row in _entropy(n, entropy)]

    def fresh_key(self) -> EdDSAPublicKey:
        return self.fresh_keys(1)[0]

    @property
    def keys(self) -> frozenset:
        return frozenset(self._pairs)

    def __contains__(self, public_key) -> bool:
        return public_key in self._pairs

    def contains_many(self, public_keys: Sequence[PublicKey]) -> List[bool]:
        return [k in self._pairs for k in public_keys]

    def sign(self, public_key: PublicKey, content) -> DigitalSignature.WithKey:
        return self.sign_many([(public_key, content)])[0]

    def sign_many(self, pairs: Sequence[Tuple[PublicKey, Union[bytes, OpaqueBytes]]]) -> List[DigitalSignature.WithKey]:
        """N x toKeyPair(pk).signWithECDSA(content): IllegalStateException for the first absent key in order."""
        for k, _ in pairs:
            if k not in self._pairs:
                raise _no_key(k)
        return [self._pairs[k].sign_with_ecdsa(_content(c)) for k, c in pairs]


class DeviceKeyManagementService:
    """The key management service on the device: a native.KeyStore of `capacity` keys (it grows by doubling when a
    batch of fresh keys would pass it).  Every method that touches private halves is ONE library call for its batch."""

    def __init__(self, engine: Optional[native.Engine] = None, capacity: int = 1024, initial_seeds: Iterable[bytes] = (),
                 device: int = 0):
        self.engine = engine or native.default_engine()
        self.store = native.KeyStore(self.engine, capacity, device)
        self._public = set()
        seeds = [bytes(s) for s in initial_seeds]
        if seeds:
            self.fresh_keys(len(seeds), b"".join(seeds))

    def close(self) -> None:
        self.store.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def fresh_keys(self, n: int, entropy=None) -> List[EdDSAPublicKey]:
        """n x freshKey() in one call; entropy: 32 bytes per key (default os.urandom).  A seed whose key the store
        already holds gives that key again."""
        if n == 0:
            return []
        seeds = _entropy(n, entropy)
        st = self.store.stats()
        if st["resident"] + n > st["capacity"]:
            self.store.reserve(max(2 * st["capacity"], st["resident"] + n))
        pk, _ = self.store.add(seeds)
        out = [EdDSAPublicKey(row.tobytes()) for row in pk]
        self._public.update(out)
        return out

    def fresh_key(self) -> EdDSAPublicKey:
        return self.fresh_keys(1)[0]

    @property
    def keys(self) -> frozenset:
        """The public halves (the reference's map has the private keys as values; those stay on the device)."""
        return frozenset(self._public)

    def contains_many(self, public_keys: Sequence[PublicKey]) -> List[bool]:
        out = [False] * len(public_keys)
        idx = [i for i, k in enumerate(public_keys) if isinstance(k, EdDSAPublicKey)]
        if idx:
            pk = np.frombuffer(b"".join(public_keys[i].encoded for i in idx), np.uint8)
            for i, f in zip(idx, self.store.contains(pk)):
                out[i] = bool(f)
        return out

    def __contains__(self, public_key) -> bool:
        return self.contains_many([public_key])[0]

    def sign(self, public_key: PublicKey, content) -> DigitalSignature.WithKey:
        return self.sign_many([(public_key, content)])[0]

    def sign_many(self, pairs: Sequence[Tuple[PublicKey, Union[bytes, OpaqueBytes]]]) -> List[DigitalSignature.WithKey]:
        """N x toKeyPair(pk).signWithECDSA(content) in one call, every record with its own key: IllegalStateException
        for the first absent key in order."""
        if not pairs:
            return []
        for k, _ in pairs:
            if not isinstance(k, EdDSAPublicKey):
                raise _no_key(k)
        pk = np.frombuffer(b"".join(k.encoded for k, _ in pairs), np.uint8)
        sig, st = self.store.sign(pk, *native.pack_blobs([_content(c) for _, c in pairs]))
        absent = np.nonzero(st != native.CV_KS_OK)[0]
        if absent.size:
            raise _no_key(pairs[int(absent[0])][0])
        return [DigitalSignature.WithKey(k, sig[j].tobytes()) for j, (k, _) in enumerate(pairs)]


def _already_signed(key: PublicKey) -> IllegalStateException:
    return IllegalStateException(f"This partial transaction was already signed by {key!r}")   # TransactionBuilder.kt:94


def _empty() -> MerkleTreeException:
    return MerkleTreeException("Cannot calculate Merkle root on empty hash list.")


def _close_builder(wtx: WireTransaction, sigs, tid: SecureHash, missing) -> Union[SignedTransaction, Exception]:
    """toSignedTransaction (TransactionBuilder.kt:132-141) once the signatures are there: missing = the mustSign
    entries the sufficiency check found unfulfilled (None: not checked)."""
    if missing:
        return IllegalStateException("Missing signatures on the transaction for the public keys: " +
                                     ", ".join(repr(k) for k in wtx.must_sign if k in missing))
    try:
        return SignedTransaction(wtx, sigs, tid)                     # require(sigs.isNotEmpty())
    except Exception as e:  # noqa: BLE001 - mirrored reference exceptions
        return e


def _finish(wtxs, results, check: bool, engine) -> list:
    """results[t]: an exception, or (sigs, id).  The sufficiency check of :133-138 for the signed transactions in one
    call (missing_signatures_batch), then the SignedTransaction or its exception per transaction."""
    missing = {}
    if check:
        signed = [t for t, r in enumerate(results) if not isinstance(r, Exception) and r[0]]
        stxs = [SignedTransaction(wtxs[t], results[t][0], results[t][1]) for t in signed]
        for t, e in zip(signed, missing_signatures_batch(stxs, (), engine)):
            missing[t] = e.missing if e is not None else None
        for t, r in enumerate(results):
            if not isinstance(r, Exception) and not r[0]:
                missing[t] = {k for k in wtxs[t].must_sign if not k.is_fulfilled_by(set())}
    return [r if isinstance(r, Exception) else _close_builder(wtxs[t], r[0], r[1], missing.get(t))
            for t, r in enumerate(results)]


def sign_transactions_batch(wtxs: Sequence[WireTransaction], keys_for_signing: Sequence[Sequence[PublicKey]], kms,
                            check_sufficient_signatures: bool = False, fused: bool = True) -> list:
    """The flows' signing loop and toSignedTransaction for many transactions: transaction t is signed with
    keys_for_signing[t], in order, by the private halves kms holds (CashFlow.kt:39-47; TransactionBuilder.kt:93-98,
    132-141).  Per transaction the SignedTransaction, or the exception the reference raises for it: IllegalStateException
    for a key kms does not hold (before signWith) or that already signed, MerkleTreeException for a transaction without
    leaves, with check_sufficient_signatures the IllegalStateException of :137, IllegalArgumentException for no
    signatures at all.  fused: ids and signatures in ONE call (cv_sign_transactions; kms must be a
    DeviceKeyManagementService); else compute_ids, a host walk of the loop and one kms.sign_many over what it signs.
    The walk is quadratic in ONE transaction's signer count (the duplicate check)."""
    if len(keys_for_signing) != len(wtxs):
        raise ValueError("keys_for_signing must have one key list per transaction")
    engine = kms.engine
    keys = [list(ks) for ks in keys_for_signing]
    results: list = [None] * len(wtxs)
    if fused:
        if not isinstance(kms, DeviceKeyManagementService):
            raise ValueError("the fused path needs a DeviceKeyManagementService")
        leaves: List[bytes] = []
        lb, sb, flat = [0], [0], []
        for t, w in enumerate(wtxs):
            leaves.extend(w.leaves)
            lb.append(len(leaves))
            # a key that is no 32-byte EdDSA key is in no store: 32 bytes no key expands to stand for it
            flat.extend(k.encoded if isinstance(k, EdDSAPublicKey) else None for k in keys[t])
            sb.append(len(flat))
        foreign = [j for j, k in enumerate(flat) if k is None]
        if foreign:
            known = kms.keys
            filler = next(bytes([i]) * 32 for i in range(256) if EdDSAPublicKey(bytes([i]) * 32) not in known)
            for j in foreign:
                flat[j] = filler
        pk = np.frombuffer(b"".join(flat), np.uint8) if flat else np.zeros(0, np.uint8)
        arena, offs, lens = native.pack_blobs(leaves)
        st, ids, sig, fb = kms.store.sign_transactions(arena, offs, lens, np.array(lb, np.uint32), pk, np.array(sb, np.uint32))
        for t, w in enumerate(wtxs):
            ks, b = keys[t], sb[t]
            if st[t] == native.CV_ST_NO_KEY:
                results[t] = _no_key(ks[int(fb[t])])
            elif st[t] == native.CV_ST_ALREADY_SIGNED:
                results[t] = _already_signed(ks[int(fb[t])])
            elif st[t] == native.CV_ST_EMPTY:
                results[t] = _empty()
            else:
                w._id = SecureHash(ids[t].tobytes())
                results[t] = ([DigitalSignature.WithKey(k, sig[b + j].tobytes()) for j, k in enumerate(ks)], w._id)
    else:
        ids = compute_ids(wtxs, engine)
        flat = [k for ks in keys for k in ks]
        have = iter(kms.contains_many(flat) if flat else [])
        pairs, owner = [], []
        for t, w in enumerate(wtxs):
            err, seen = None, []
            for k, present in zip(keys[t], [next(have) for _ in keys[t]]):
                if err is not None:
                    continue
                if not present:
                    err = _no_key(k)
                elif k in seen:
                    err = _already_signed(k)
                elif ids[t] is None:
                    err = _empty()
                seen.append(k)
            if err is None and ids[t] is None:
                err = _empty()
            if err is not None:
                results[t] = err
            else:
                results[t] = ([], ids[t])
                pairs.extend((k, ids[t].bytes) for k in keys[t])
                owner.extend([t] * len(keys[t]))
        for t, s in zip(owner, kms.sign_many(pairs)):
            results[t][0].append(s)
    return _finish(wtxs, results, check_sufficient_signatures, engine)
