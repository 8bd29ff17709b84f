"""Cases and the reference for the device key dedupe (corda_amd/csrc/cv_keydedupe.h), shared by
tests/test_keydedupe_cpu.py (the lane functions on the CPU) and tests/test_gpu_keydedupe.py (the entry point
cv_ed25519_dedupe_keys_device on the GPU).  Pure Python and numpy.

The reference is first-seen numbering over `bytes` rows: a dict from a key's 32 bytes to the number of distinct keys
seen before it, the numbering cv_diag_dedupe_keys documents.  Two keys are equal iff their 32 bytes are.
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def reference(pk):
    """pk[n][32] uint8 -> (keys[nkeys][32] uint8, key_index[n] uint32, nkeys)."""
    seen, keys, index = {}, [], []
    for b in np.ascontiguousarray(pk, np.uint8).reshape(-1, 32).view("V32").ravel().tolist():     # the rows as bytes
        if b not in seen:
            seen[b] = len(keys)
            keys.append(b)
        index.append(seen[b])
    return (np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32).copy(), np.array(index, np.uint32), len(keys))


def key(*tag) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(repr(tag).encode()).digest(), np.uint8).copy()


def pool(tag, k) -> np.ndarray:
    return np.array([key(tag, j) for j in range(k)], np.uint8)


def signed_pool_rows(n):
    """n rows drawn as resolve_cases._signed draws a chain's signers: four keys, who = (i * 7 // 3) % 4."""
    keys = np.array([np.frombuffer(hashlib.sha256(b"key %d" % k).digest(), np.uint8) for k in range(4)])
    return keys[(np.arange(n) * 7 // 3) % 4].copy()


def bad_key_rows():
    """The golden corpus's rows whose key is no point, each three times, interleaved with two good keys."""
    z = np.load(os.path.join(GOLDEN, "ed25519_corpus.npz"))
    bad = z["pk"][z["status"] == 1]
    assert len(bad) >= 2
    good = pool("good", 2)
    rows = []
    for r in range(3):
        for j, b in enumerate(bad):
            rows += [b, good[(j + r) % 2]]
    return np.array(rows, np.uint8)


def _variants(tag, byte, k, n):
    """n rows of k keys that are one key but for `byte`."""
    base = key(tag)
    ks = np.tile(base, (k, 1))
    ks[:, byte] = (base[byte] + 1 + np.arange(k)) & 0xFF
    return ks[np.random.default_rng(k * 1000 + n).integers(0, k, n)].copy()


def cases():
    """-> {name: pk[n][32]}; every array is the case's own."""
    rng = np.random.default_rng(20261021)
    c = {}
    c["n1"] = pool("one", 1)
    c["n2_equal"] = np.tile(key("two"), (2, 1))
    c["n2_different"] = pool("two", 2)
    for n in (63, 64, 65):
        c[f"n{n}"] = pool(n, 9)[rng.integers(0, 9, n)].copy()
    c["all_equal"] = np.tile(key("same"), (300, 1))
    c["all_distinct"] = pool("distinct", 300)
    c["alternating"] = pool("alt", 2)[np.arange(301) % 2].copy()
    c["differ_in_byte_31"] = _variants("b31", 31, 5, 200)         # words 0-6 equal
    c["differ_in_byte_0"] = _variants("b0", 0, 5, 200)            # bytes 1-31 equal
    rows = pool("fal", 6)[rng.integers(0, 6, 130)]
    c["first_occurrence_at_the_last_index"] = np.concatenate([rows, key("fal", "new")[None]])
    rows = pool("ral", 6)[rng.integers(0, 6, 130)].copy()
    rows[17] = key("ral", "twice")
    c["only_repeat_at_the_last_index"] = np.concatenate([rows, key("ral", "twice")[None]])
    c["signed_pool_of_4"] = signed_pool_rows(5000)
    c["bad_keys_repeated"] = bad_key_rows()
    return c


def words(pk) -> np.ndarray:
    """The rows as the uint32 words the lanes read (a copy, aligned)."""
    return np.ascontiguousarray(pk, np.uint8).reshape(-1).view(np.uint32).copy()
