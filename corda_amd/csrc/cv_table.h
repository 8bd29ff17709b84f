// cv_table.h — what every device hash table of the library shares: the atomics that reduce to plain operations on the
// CPU, the seeded hash of a 32-byte key, ONE bounded probe walk and ONE size function.  __host__ __device__: the
// kernels' per-lane cores (cv_uniq.h, cv_keystore.h, cv_keydedupe.h, cv_resolve.h) and the CPU harnesses of tests/
// compile the same text; tests/table_san.cpp runs the walk and the size function alone.
//
// EVERY TABLE is open addressing with linear probing over a power-of-two slot count of at least twice its entries
// (cv_table_slots), the slot chosen by cvu_hash's seeded mix of all eight key words (keys are bytes a submitter can
// grind: no key bits choose a slot directly), and nothing is ever deleted, so a probe ends at the first empty slot.
// A probe is cv_walk with a visitor: the walk owns the bound (mask + 1 slots), the step and the wrap count; the
// visitor owns what a slot means — who looks before the CAS, who lowers with atomicMin, who wins.  Those differences
// are behaviour and stand, one line each, at the call sites (DESIGN.md §5.17 lists them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef CV_HD
#define CV_HD __host__ __device__ __forceinline__
#endif

CV_HD uint32_t cvu_atomic_cas(uint32_t *p, uint32_t expect, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    return atomicCAS(p, expect, v);
#else
    const uint32_t old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}
CV_HD void cvu_atomic_min(uint32_t *p, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
CV_HD void cvu_atomic_add(uint32_t *p, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
// a running maximum: the plain read first spares most lanes the atomic (the word only grows)
CV_HD void cvu_note_max(uint32_t *p, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    if (v > *p) atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}
// an atomic read of a slot other lanes of the kernel change (relaxed: any value the slot has held will do)
CV_HD uint32_t cvd_atomic_load(const uint32_t *p) {
#ifdef __HIP_DEVICE_COMPILE__
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}

CV_HD uint64_t cvu_mix64(uint64_t x) {
    x ^= x >> 32;
    x *= 0xd6e8feb86659fd93ull;
    x ^= x >> 29;
    x *= 0x9e3779b97f4a7c15ull;
    x ^= x >> 32;
    return x;
}

// all eight key words folded with the seed; the low bits choose the slot, the high word is the fingerprint
CV_HD uint64_t cvu_hash(const uint32_t *k, uint64_t seed) {
    uint64_t h = seed;
#pragma unroll
    for (int q = 0; q < 4; q++) h = cvu_mix64(h ^ ((uint64_t)k[2 * q] | ((uint64_t)k[2 * q + 1] << 32))) + seed;
    return h;
}
CV_HD uint32_t cvu_tag(uint64_t h) { return (uint32_t)(h >> 32) | 1u; }

CV_HD bool cvu_key_eq(const uint32_t *a, const uint32_t *b) {
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) diff |= a[q] ^ b[q];
    return diff == 0;
}
CV_HD void cvu_copy8(uint32_t *d, const uint32_t *s) {
#pragma unroll
    for (int q = 0; q < 8; q++) d[q] = s[q];
}
// eight words between 16-byte aligned places (a table's arrays and a call's buffers are): two 16-byte moves on the device
CV_HD void cvu_copy8_aligned(uint32_t *d, const uint32_t *s) {
#ifdef __HIP_DEVICE_COMPILE__
    d = static_cast<uint32_t *>(__builtin_assume_aligned(d, 16));
    s = static_cast<const uint32_t *>(__builtin_assume_aligned(s, 16));
#endif
    cvu_copy8(d, s);
}

// Slots of a table of n entries: the power of two that is at least `floor` (a power of two) and at least 2 n.
CV_HD uint64_t cv_table_slots(uint64_t n, uint64_t floor) {
    uint64_t s = floor;
    while (s < 2 * n) s <<= 1;
    return s;
}

// THE PROBE: visit(slot) for slot = start & mask, then the next slot, wrapping after slot `mask`, until the visitor
// returns non-zero (stop) or mask + 1 slots were looked at — never more.  The walk hands back n, the slots looked at,
// `stopped`, what the visitor stopped it with (0: it ran out), and the slot it stopped at: values, so that a visitor
// need capture nothing by reference.  Leaving slot `mask` without a stop adds one to *wraps (null: not counted, nothing
// written).  I: uint32_t, or uint64_t for a table that may pass 2^32 slots.
template <class I> struct CvWalk {
    I n, slot;
    int stopped;
};
template <class I, class F> CV_HD CvWalk<I> cv_walk(I mask, I start, uint32_t *wraps, F visit) {
    I slot = start & mask, n = 0;
    while (n <= mask) {
        n++;
        const int stop = visit(slot);
        if (stop) return {n, slot, stop};
        if (wraps && slot == mask) cvu_atomic_add(wraps, 1);
        slot = (slot + 1) & mask;
    }
    return {n, slot, 0};
}

// THE RESIDENT TABLES (the uniqueness set, the key store) keep 0 or the key's tag in occ and the key beside it;
// key_at(slot) reaches a slot's eight key words.  Words 0 and 1 of their per-call device counters are the same:
#define CVT_D_ERROR 0             // a probe ran out of slots
#define CVT_D_MAXPROBE 1          // longest probe of the resident table (slots looked at)
#define CVT_NONE 0xffffffffu      // no slot
#define CVT_EMPTY 1               // what their visitors stop a walk with: an empty slot / the key's (or the claimed) slot
#define CVT_HIT 2

// after a resident walk: the error word when it ran out (the capacity check rules it out), the longest probe
CV_HD void cvt_note(uint32_t *dstat, const CvWalk<uint32_t> &w) {
    if (!w.stopped) dstat[CVT_D_ERROR] = 1;
    cvu_note_max(dstat + CVT_D_MAXPROBE, w.n);
}

// The slot holding `key` (hash h), or CVT_NONE.  Read-only; the tag is compared before the key.
template <class K>
CV_HD uint32_t cvt_find(const uint32_t *occ, uint32_t mask, K key_at, const uint32_t *key, uint64_t h, uint32_t *dstat,
                        uint32_t *wraps) {
    const uint32_t tag = cvu_tag(h);
    const CvWalk<uint32_t> w = cv_walk(mask, (uint32_t)h, wraps, [=](uint32_t slot) {
        const uint32_t o = occ[slot];
        return o == 0 ? CVT_EMPTY : (o == tag && cvu_key_eq(key_at(slot), key)) ? CVT_HIT : 0;
    });
    cvt_note(dstat, w);
    return w.stopped == CVT_HIT ? w.slot : CVT_NONE;
}

// For a key that is absent and that no other lane inserts: the walk to the first slot this lane's CAS turns from
// empty to the tag, without a key compare (stopped: w.slot is claimed).  The caller stores the slot's payload with
// plain stores and then calls cvt_note, the order the memory operations have always had.
CV_HD CvWalk<uint32_t> cvt_claim(uint32_t *occ, uint32_t mask, uint64_t h, uint32_t *wraps) {
    const uint32_t tag = cvu_tag(h);
    return cv_walk(mask, (uint32_t)h, wraps,
                   [=](uint32_t slot) { return cvu_atomic_cas(occ + slot, 0u, tag) == 0u ? CVT_HIT : 0; });
}
