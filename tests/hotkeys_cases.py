"""Cases and the reference for the hot-key route (corda_amd/csrc/cv_hotkeys.h), shared by tests/test_hotkeys_cpu.py (the
lane functions on the CPU) and tests/test_gpu_hotkeys.py (cv_ed25519_verify_device_hotkeys on the GPU).  Pure Python
and numpy.

The reference restates the classification of DESIGN.md §5.15 over keydedupe_cases.reference: keys numbered in
first-seen order, a key a candidate iff it occurs at least hot_min times, hot iff it is among the first hot_cap
candidates in first-seen order, and the stable partition of the records: hot ones first, each class in input order.
"""
import numpy as np

import keydedupe_cases as K

COLD = 0xFFFFFFFF
CAP = 16384                     # the key pool's default capacity


def reference(pk, hot_min, hot_cap=CAP):
    """pk[n][32] -> (cls[nkeys] uint32: a hot key's number among the hot keys, COLD for a cold key; hotnum[nkeys]: the
    candidates before each key; perm[n]: each record's row in the partitioned batch; nhot: the hot records)."""
    hot_min = hot_min or 8
    _, index, nk = K.reference(pk)
    count = np.bincount(index, minlength=nk)
    cand = count >= hot_min
    hotnum = (np.cumsum(cand) - cand).astype(np.uint32)
    hot = cand & (hotnum < hot_cap)
    cls = np.where(hot, hotnum, COLD).astype(np.uint32)
    rec_hot = hot[index]
    nhot = int(rec_hot.sum())
    perm = np.empty(len(index), np.uint32)
    perm[rec_hot] = np.arange(nhot, dtype=np.uint32)
    perm[~rec_hot] = nhot + np.arange(len(index) - nhot, dtype=np.uint32)
    return cls, hotnum, perm, nhot


def route(pk, hot_min, hot_cap=CAP):
    """What route_out reports: (nkeys, hot keys, hot records, cold records)."""
    cls, _, _, nhot = reference(pk, hot_min, hot_cap)
    return len(cls), int((cls != COLD).sum()), nhot, len(pk) - nhot


def _occurrences(tag, counts, seed):
    """Key j of a fresh pool counts[j] times, the rows shuffled."""
    p = K.pool(tag, len(counts))
    rows = np.repeat(p, counts, axis=0)
    return rows[np.random.default_rng(seed).permutation(len(rows))].copy()


def cases():
    """-> {name: (pk[n][32], hot_min, hot_cap)}: every case of keydedupe_cases under hot_min 1, 2, 8 and n + 1, then
    the route's own."""
    c = {}
    for name, pk in K.cases().items():
        for hm in (1, 2, 8, len(pk) + 1):
            c[f"{name}/min{hm}"] = (pk, hm, CAP)
    for hm in (2, 3, 8):
        # exactly hot_min - 1, hot_min and hot_min + 1 occurrences, among keys seen once
        c[f"around_min{hm}"] = (_occurrences(("around", hm), [hm - 1, hm, hm + 1, 1, 1, 1], hm), hm, CAP)
    rows = K.pool("first0", 40)
    hot = K.key("first0", "hot")
    c["first_hot_record_at_index_0"] = (np.concatenate([hot[None], rows, np.tile(hot, (4, 1))]), 3, CAP)
    # the hot key's occurrences lie at the end: the first hot record is the last but two, the last record is hot
    c["hot_records_at_the_end"] = (np.concatenate([rows, np.tile(hot, (3, 1))]), 3, CAP)
    # a key that occurs once, at n - 1, under hot_min 1: the first (and only) record of the last hot key
    c["first_hot_record_at_the_last_index"] = (np.concatenate([np.tile(hot, (70, 1)), K.key("first0", "last")[None]]), 1, CAP)
    c["more_candidates_than_cap"] = (_occurrences("cap", [3, 1, 4, 2, 5, 1, 2, 6, 2, 3, 1, 2], 7), 2, 4)
    c["cap_1"] = (_occurrences("cap1", [2, 2, 2, 1], 8), 2, 1)
    c["default_min"] = (_occurrences("def", [7, 8, 9, 1, 1], 9), 0, CAP)
    c["past_two_blocks"] = (K.pool("hblocks", 700)[np.random.default_rng(5).integers(0, 700, 2500)].copy(), 4, CAP)
    return c
