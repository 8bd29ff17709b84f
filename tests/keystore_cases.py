"""Shared cases of the key store's tests (tests/test_keystore_cpu.py, tests/test_gpu_keystore*.py): a literal
restatement of the flows' signing loop — sign_ref — and the batches the tests run through it.

Reference: CashFlow.kt:39-47 (keysForSigning.keys.forEach { keys[it] ?: throw ...; builder.signWith(KeyPair(it, key)) }),
TransactionBuilder.kt:93-98 (signWith: check(currentSigs.none { it.by == key.public }); toWireTransaction().id;
signWithECDSA) and :132-141 (toSignedTransaction computes wtx.id), Services.kt:206-212 (toPrivate).
"""
import hashlib

import numpy as np

ST_OK, ST_NO_KEY, ST_ALREADY_SIGNED, ST_EMPTY = 0, 1, 2, 3
NO_BAD = 0xFFFFFFFF
KS_ADDED, KS_PRESENT, KS_OK, KS_NO_KEY = 0, 1, 0, 1


def merkle_id(leaves) -> bytes:
    """WireTransaction.id: the Merkle root of the leaves' SHA-256 hashes, the last hash of an odd level doubled
    (MerkleTransaction.kt:66-99); 32 zero bytes for no leaves (the library's rule for the id of CV_TX_EMPTY)."""
    lvl = [hashlib.sha256(bytes(x)).digest() for x in leaves]
    if not lvl:
        return bytes(32)
    while len(lvl) > 1:
        lvl = [hashlib.sha256(lvl[i] + (lvl[i + 1] if i + 1 < len(lvl) else lvl[-1])).digest() for i in range(0, len(lvl), 2)]
    return lvl[0]


def sign_ref(store, txs, sign, id_of=merkle_id):
    """store: {public key bytes: seed}; txs: [(leaves, keys)]; sign(seed, message) -> 64 bytes.  Per transaction
    (status, first_bad, id, [signature per key]): per key in order lookup -> duplicate check -> id -> sign; a
    transaction that fails anywhere is abandoned, all of its signatures zero."""
    out = []
    for leaves, keys in txs:
        tid = id_of(leaves)
        status, bad, sigs, signed = ST_OK, NO_BAD, [], []
        for j, k in enumerate(keys):
            if k not in store:                                   # keys[it] ?: throw IllegalStateException
                status, bad = ST_NO_KEY, j
                break
            if k in signed:                                      # check(currentSigs.none { it.by == key.public })
                status, bad = ST_ALREADY_SIGNED, j
                break
            if not leaves:                                       # toWireTransaction().id: MerkleTreeException
                status, bad = ST_EMPTY, j
                break
            sigs.append(sign(store[k], tid))
            signed.append(k)
        if status == ST_OK and not leaves:                       # no keys: toSignedTransaction computes wtx.id
            status, bad = ST_EMPTY, 0
        if status != ST_OK:
            sigs = [bytes(64)] * len(keys)
        out.append((status, bad, tid, sigs))
    return out


def flatten_txs(txs):
    """[(leaves, keys)] -> (leaves back to back, tx_leaf_begin, pk (nsig, 32) u8, tx_sig_begin)."""
    blobs, lb, keys, sb = [], [0], [], [0]
    for leaves, ks in txs:
        blobs.extend(bytes(x) for x in leaves)
        lb.append(len(blobs))
        keys.extend(ks)
        sb.append(len(keys))
    pk = np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32).copy() if keys else np.zeros((0, 32), np.uint8)
    return blobs, np.array(lb, np.uint32), pk, np.array(sb, np.uint32)


def precedence_txs(present, absent, leaf=lambda i: b"leaf-%d" % i):
    """The status precedence cases, each named: present = at least 3 resident keys, absent = at least 2 keys the
    store does not hold."""
    p, a = present, absent
    L = [leaf(0), leaf(1), leaf(2)]
    return {
        "ok_one": (L[:1], [p[0]]),
        "ok_three": (L, [p[0], p[1], p[2]]),
        "ok_no_keys": (L[:2], []),
        "empty_no_keys": ([], []),
        "empty_key0_absent": ([], [a[0], p[0]]),                 # NO_KEY at 0: thrown before signWith
        "empty_key0_present": ([], [p[0], a[0]]),                # EMPTY at 0: inside the first signWith
        "no_key_first": (L, [a[0], p[0]]),
        "no_key_last": (L, [p[0], p[1], a[1]]),
        "dup_adjacent": (L, [p[0], p[0]]),
        "dup_far": (L, [p[0], p[1], p[2], p[0]]),
        "dup_of_absent": (L, [a[0], a[0]]),                      # NO_KEY at 0: the lookup comes first
        "no_key_before_dup": (L, [p[0], a[0], p[0]]),            # key 2 repeats key 0, key 1 is absent: NO_KEY at 1
        "dup_before_no_key": (L, [p[0], p[0], a[0]]),            # ALREADY_SIGNED at 1
        "empty_dup": ([], [p[1], p[1]]),                         # EMPTY at 0: the walk stops in the first signWith
    }


PRECEDENCE_EXPECT = {
    "ok_one": (ST_OK, NO_BAD), "ok_three": (ST_OK, NO_BAD), "ok_no_keys": (ST_OK, NO_BAD),
    "empty_no_keys": (ST_EMPTY, 0), "empty_key0_absent": (ST_NO_KEY, 0), "empty_key0_present": (ST_EMPTY, 0),
    "no_key_first": (ST_NO_KEY, 0), "no_key_last": (ST_NO_KEY, 2), "dup_adjacent": (ST_ALREADY_SIGNED, 1),
    "dup_far": (ST_ALREADY_SIGNED, 3), "dup_of_absent": (ST_NO_KEY, 0), "no_key_before_dup": (ST_NO_KEY, 1),
    "dup_before_no_key": (ST_ALREADY_SIGNED, 1), "empty_dup": (ST_EMPTY, 0),
}


def random_txs(rng, ntx, present, absent):
    """ntx transactions of 0-5 leaves and 0-4 keys over the resident keys, one in four with a fault: an absent key,
    a repeated key, or no leaves."""
    txs = []
    for t in range(ntx):
        leaves = [rng.bytes(int(rng.integers(1, 120))) for _ in range(int(rng.integers(0, 6)))]
        nk = int(rng.integers(0, 5))
        keys = [present[int(i)] for i in rng.choice(len(present), size=nk, replace=False)]
        fault = int(rng.integers(0, 8))
        if fault == 0 and nk:
            keys[int(rng.integers(0, nk))] = absent[int(rng.integers(0, len(absent)))]
        elif fault == 1 and nk >= 2:
            keys[nk - 1] = keys[int(rng.integers(0, nk - 1))]
        txs.append((leaves, keys))
    return txs
