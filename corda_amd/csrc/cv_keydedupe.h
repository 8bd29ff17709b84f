// cv_keydedupe.h — the distinct public keys of a batch of signatures, found on the device: pk[n][32] -> nkeys,
// keys[nkeys][32] in FIRST-SEEN order (the numbering cv_diag_dedupe_keys documents) and key_index[n], what the keyed
// verify path (cv_k_keyed.hip) takes.  Two keys are equal iff all 32 bytes are equal; nothing is decoded, so a
// non-canonical encoding of a point is a key of its own, as in the key pool.  The per-lane core of cv_k_dedupe.hip;
// __host__ __device__, so tests/keydedupe_harness.cpp runs the lanes on the CPU one after another, in any order (the
// atomics reduce to plain operations there).
//
// ONE dedupe, a kernel per step, no lane reading what another lane of its kernel writes except through an atomic:
//   insert  per signature i: atomicCAS(slot, NONE, i) into a call-local table of signature INDICES (a table of
//           cv_table.h: probing, sizing and hashing are described there; a floor of 2 slots).  A loser compares
//           pk[occupant] with pk[i] — both in the immutable input — and probes on, or, on equality, does
//           atomicMin(slot, i): the slot ends at the key's FIRST occurrence, whichever lane won.  Two things keep
//           the lanes of a batch of few keys off each other's atomics (all of one address run one after another): a
//           lane first reads the slot atomically and leaves a holder with its key and a smaller index alone, and in
//           the kernel lanes of a wave that carry the key of a lower lane of that wave leave the insert to it (a few
//           election rounds, cv_k_dedupe.hip; the lower lane's index is the smaller one, so the slot's final value is
//           the same with and without them, which is why the CPU harness can run every lane through cvd_insert).
//   mark    per signature i, the table read-only by then (the kernel boundary publishes it): first[i] = the value of
//           its key's slot; number[i] = (first[i] == i), the flag of a first occurrence.
//   count   per block of CVD_SPAN entries: the block's sum                     } the ordered compaction of the flags:
//   scan    per block of CVD_SPAN entries: its exclusive prefix sums in place, } number[i] becomes the flags before i,
//           from the block's base (the scanned block sums) when there is one   } one more level of count and scan per
//                                                                              } factor CVD_SPAN of n; STAT_TOTAL = nkeys
//   emit    per signature i: key_index[i] = number[first[i]]; a first occurrence writes keys[number[i]] = pk[i]; lane
//           0 writes *nkeys.
// THE RESULT IS A FUNCTION OF THE INPUT BYTES ALONE.  Which slot a key lands in depends on the seed and on which lanes
// ran first, but the slot's final value does not: every lane that carries the key either claims the slot or lowers it
// with atomicMin, so it ends at the smallest index with that key.  first[], the flags, their prefix sums (index order)
// and so keys, key_index and nkeys follow from that alone.
// NO LANE WAITS FOR ANOTHER LANE: no spin, lock or flag.  EVERY PROBE IS BOUNDED: each is cv_walk (cv_table.h), which
// looks at no more than the slot count, and clears stat[CVD_STAT_OK] when it runs out; emit then reports
// nkeys = CVD_NONE (no batch has that many keys) and a host that reads the count back returns CV_E_HIP.  The slot
// count rules it out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cv_uniq.h"

#define CVD_NONE 0xffffffffu       // an empty slot; nkeys after a probe error
#define CVD_PER 4u                 // entries per lane of the compaction's kernels
#define CVD_SPAN 1024u             // entries per block of them: CV_BLOCK lanes x CVD_PER
#define CVD_LEVELS 3               // levels of block sums: n < 2^32 <= CVD_SPAN^4
// words of stat, which lies behind the table: ONE memset of 0xff clears the table and sets STAT_OK
#define CVD_STAT_OK 0              // CVD_NONE until a probe loop runs out of slots
#define CVD_STAT_TOTAL 1           // the distinct keys (the scan of the last level writes it)
#define CVD_STAT_WORDS 4

struct CvDedupe {
    uint32_t n;
    const uint32_t *pk;            // n * 8: the words of the key bytes
    uint32_t *tab;                 // mask + 1 slots, CVD_NONE = empty
    uint64_t mask, seed;           // 64 bits: 2 n slots pass 2^32 from n = 2^31
    uint32_t *stat;                // CVD_STAT_WORDS
    uint32_t *first, *number;      // n each
    uint32_t *keys, *key_index, *nkeys;
};

CV_HD void cvd_insert(const CvDedupe &D, uint32_t i) {
    const uint32_t *k = D.pk + 8 * (size_t)i;
    // the relaxed look BEFORE the CAS, the CAS only when it read empty; atomicMin only when i < old (first occurrence)
    const CvWalk<uint64_t> w = cv_walk(D.mask, cvu_hash(k, D.seed), nullptr, [&](uint64_t slot) {
        // A look before the read-modify-write: a batch of few keys sends thousands of lanes to one slot, and the
        // atomics of one address run one after another.  A slot, once claimed, keeps its key and only falls, so
        // whatever value the look gives, a holder with this lane's key at or below i means i cannot be the slot's
        // final value: nothing to do.
        uint32_t old = cvd_atomic_load(D.tab + slot);
        if (old == CVD_NONE) old = cvu_atomic_cas(D.tab + slot, CVD_NONE, i);
        if (old == CVD_NONE) return true;
        // `old` may already have been lowered by another lane with the same key: any holder of the slot carries it
        if (!cvu_key_eq(D.pk + 8 * (size_t)old, k)) return false;
        if (i < old) cvu_atomic_min(D.tab + slot, i);
        return true;
    });
    if (!w.stopped) D.stat[CVD_STAT_OK] = 0;    // more signatures than slots: the caller sized the table at twice
}

CV_HD void cvd_mark(const CvDedupe &D, uint32_t i) {
    const uint32_t *k = D.pk + 8 * (size_t)i;
    uint32_t f = CVD_NONE;
    // read-only, the o < D.n guard kept; an empty slot ends the walk WITHOUT a holder, an error as f > i is
    cv_walk(D.mask, cvu_hash(k, D.seed), nullptr, [&](uint64_t slot) {
        const uint32_t o = D.tab[slot];
        if (o == CVD_NONE) return true;         // insert put the key before this slot: only after its probe error
        if (o >= D.n || !cvu_key_eq(D.pk + 8 * (size_t)o, k)) return false;
        f = o;
        return true;
    });
    if (f > i) {                                // no holder (CVD_NONE), or one after i: a key of its own, every index in range
        D.stat[CVD_STAT_OK] = 0;
        f = i;
    }
    D.first[i] = f;
    D.number[i] = f == i;
}

CV_HD void cvd_emit(const CvDedupe &D, uint32_t i) {
    const uint32_t f = D.first[i], k = D.number[f];
    D.key_index[i] = k;
    if (f == i) cvu_copy8(D.keys + 8 * (size_t)k, D.pk + 8 * (size_t)i);
    if (i == 0) *D.nkeys = D.stat[CVD_STAT_OK] == CVD_NONE ? D.stat[CVD_STAT_TOTAL] : CVD_NONE;
}

// ---------------------------------------------------------------- host: the workspace
#ifndef __HIP_DEVICE_COMPILE__
// slots of the table: a power of two, at least 2 n (n < 2^32)
inline uint64_t cvd_slots(uint64_t n) { return cv_table_slots(n, 2); }
inline uint64_t cvd_blocks(uint64_t m) { return (m + CVD_SPAN - 1) / CVD_SPAN; }

// Offsets into the workspace, each piece 16-byte aligned: table | stat | first | number | the levels' block sums
struct CvdLayout {
    uint64_t slots, tab, stat, first, number, sum[CVD_LEVELS], bytes;
};
inline CvdLayout cvd_layout(uint64_t n) {
    auto al = [](uint64_t x) { return (x + 15) & ~(uint64_t)15; };
    CvdLayout L{};
    L.slots = cvd_slots(n);
    L.tab = 0;
    L.stat = L.tab + 4 * L.slots;
    L.first = L.stat + al(4 * CVD_STAT_WORDS);
    L.number = L.first + al(4 * n);
    uint64_t top = L.number + al(4 * n), m = n;
    for (int k = 0; k < CVD_LEVELS; k++) {
        m = cvd_blocks(m);
        L.sum[k] = top;
        top += al(4 * m);
    }
    L.bytes = top;
    return L;
}
inline CvDedupe cvd_args(uint64_t n, const void *pk, void *keys, void *key_index, void *nkeys, void *ws, uint64_t seed,
                         const CvdLayout &L) {
    uint8_t *w = static_cast<uint8_t *>(ws);
    CvDedupe D{};
    D.n = (uint32_t)n, D.pk = static_cast<const uint32_t *>(pk);
    D.tab = reinterpret_cast<uint32_t *>(w + L.tab), D.mask = L.slots - 1, D.seed = seed;
    D.stat = reinterpret_cast<uint32_t *>(w + L.stat);
    D.first = reinterpret_cast<uint32_t *>(w + L.first), D.number = reinterpret_cast<uint32_t *>(w + L.number);
    D.keys = static_cast<uint32_t *>(keys), D.key_index = static_cast<uint32_t *>(key_index);
    D.nkeys = static_cast<uint32_t *>(nkeys);
    return D;
}
#endif
