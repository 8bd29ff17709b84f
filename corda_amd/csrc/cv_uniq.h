// cv_uniq.h — the notary's uniqueness set: UniquenessProvider.commit (core/src/main/kotlin/net/corda/core/node/
// services/UniquenessProvider.kt:13-35) as InMemoryUniquenessProvider decides it (node/.../transactions/
// InMemoryUniquenessProvider.kt:14-36; the decision half of PersistentUniquenessProvider.kt:61-81), for a whole batch
// of requests, decided EXACTLY as that many sequential commit calls in request order.  The per-lane core of
// cv_k_uniq.hip; __host__ __device__, so tests/uniq_harness.cpp runs the lanes on the CPU one after another, in any
// order (the atomics reduce to plain operations there).
//
// RESIDENT TABLE (CvUniqTable): a table of cv_table.h (probing, sizing and hashing are described there) with a
// per-set random seed and a floor of 16 slots, structure of arrays: occ (0 = empty, else the tag: a 32-bit fingerprint
// of the key's hash with bit 0 set), key (8 words), id (8 words), index, caller.
//
// ONE commit_batch (ntx requests, request t holding states [begin[t], begin[t + 1])), a kernel per step:
//   init    per request: stat = UNDECIDED, or REJECTED when its enable byte is 0; state_tx of its states
//   group   per state i: atomicCAS(btab slot, EMPTY, i) into a batch-local table of state INDICES; the winner is the
//           representative of its key (rep[i] = i), a loser compares key[old] with key[i] — both in the immutable
//           input — and takes rep[i] = old or probes on.  Then the resident table (read-only here): a hit sets
//           res[i] = the slot and stat[state_tx[i]] = REJECTED.
//   rounds  owner[.] = NONE; claim: every request that is not REJECTED does atomicMin(owner[rep(s)], t); decide:
//           every UNDECIDED request reads the statuses of BEFORE the round (two status arrays alternate) and becomes
//           ACCEPTED if it owns all its states, REJECTED if one of them is owned by an ACCEPTED smaller request, else
//           stays.  Both verdicts are the sequential ones: owning everything means every earlier holder was rejected;
//           an accepted earlier owner is a conflict.  The smallest undecided request is decided each round (all
//           earlier ones are decided, so each of its states is its own or an accepted request's).
//   own     owner[.] = NONE, then every ACCEPTED request stores owner[rep(s)] = t and last[rep(s)] = the input index
//           (ascending, so the last index wins; no two accepted requests share a key, so no two lanes share a word)
//   tail    ONE lane walks the requests still UNDECIDED in order: REJECTED if a state has an owner other than
//           itself (an accepted one, and then a smaller one), else ACCEPTED and it takes ownership as `own` does
//   report  per request: SKIPPED | OK (state_conflict 0, one insert per distinct key: the state with
//           last[rep] == its index) | CONFLICT (state s reported iff res[s] is a slot — the record is the slot's — or
//           owner[rep(s)] < t — the record is the owner's id, last[rep(s)] and the owner's caller)
// An inserted key is known absent and distinct from every other key inserted by the call, so the insert claims the
// first slot whose atomicCAS(occ, 0, tag) succeeds, without a key compare, and writes key and record with plain
// stores; the kernel boundary publishes them (no lane of the inserting kernel reads a slot that was empty before it).
//
// SNAPSHOT (DistributedImmutableMap.snapshot): an ordered stream compaction of the occupied slots of a window
// [slot_begin, slot_end) of the resident table, one lane per slot, the table read-only:
//   count   per block: the occupied slots of its lanes (a ballot and a popcount per wave, the wave totals through LDS)
//   scan    the block totals -> their exclusive prefix sums and the window's total (the key dedupe's hierarchical scan)
//   emit    an occupied slot's rank r = block base + the waves before it + the lanes before it, so ranks ascend with
//           the slot: r < max_entries writes record r (key, id, index, caller: the committed words), r == max_entries
//           stores its slot as the next cursor; one lane closes: count = min(total, max_entries), and the next cursor
//           is slot_end when no lane has rank max_entries.  Every output word has exactly one writer.
// The records are a function of the table and the window alone.  INSTALL builds a fresh table with the load path
// (cvu_group with stat == null, cvu_load_check, cvu_load_put) and the host swaps the tables; CLEAR zeroes occ.
//
// NO LANE WAITS FOR ANOTHER LANE: no spin, lock or flag.  EVERY PROBE IS BOUNDED: each is cv_walk (cv_table.h), which
// looks at no more than its table's slot count, and sets dstat[CVU_D_ERROR] when it runs out (the host returns
// CV_E_HIP).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cv_table.h"

#define CVU_NONE CVT_NONE         // empty batch slot, no owner, not resident
#define CVU_UNDECIDED 0u
#define CVU_ACCEPTED 1u
#define CVU_REJECTED 2u
// tx_status (include/cordaverify.h CV_UNIQ_*)
#define CVU_OK 0
#define CVU_CONFLICT 1
#define CVU_SKIPPED 2
// words of the per-call device counters
#define CVU_D_ERROR CVT_D_ERROR    // a probe ran out of slots
#define CVU_D_MAXPROBE CVT_D_MAXPROBE   // longest probe of the resident table (slots looked at)
#define CVU_D_WRAPS 2             // probes of the resident table that passed its last slot
#define CVU_D_INSERTED 3
#define CVU_D_TAIL 4              // requests the serial tail decided
#define CVU_D_BAD 5               // load: a key repeated in the call or already resident
#define CVU_D_ROUND0 8            // [CVU_D_ROUND0 + r]: requests undecided after round r
#define CVU_MAX_ROUNDS 64
#define CVU_D_WORDS (CVU_D_ROUND0 + CVU_MAX_ROUNDS)

struct CvUniqTable {
    uint32_t *occ, *key, *id, *index, *caller;
    uint32_t mask;                // slots - 1
    uint64_t seed;
};
#ifndef __HIP_DEVICE_COMPILE__
// the table in ONE allocation of CVU_SLOT_BYTES * slots at base: occ | key | id | index | caller
#define CVU_SLOT_BYTES 76
inline CvUniqTable cvu_carve(void *base, size_t slots, uint64_t seed) {
    uint32_t *p = static_cast<uint32_t *>(base);
    return CvUniqTable{p, p + slots, p + 9 * slots, p + 17 * slots, p + 18 * slots, (uint32_t)(slots - 1), seed};
}
#endif

// words of a snapshot call's device result
#define CVU_SNAP_NEXT 0           // the slot the next call starts at (slot_end: the window is done)
#define CVU_SNAP_COUNT 1          // records written: min(total, max_entries)
#define CVU_SNAP_TOTAL 2          // occupied slots of the window (the scan writes it)
#define CVU_SNAP_WORDS 4

struct CvUniqSnap {
    uint32_t slot_begin, slot_end;                // the window, slot_end <= the slot count
    uint32_t max_entries;                         // at least 1
    uint32_t *key, *id, *index, *caller;          // min(max_entries, slot_end - slot_begin) records
    uint32_t *out;                                // CVU_SNAP_WORDS
};

struct CvUniqBatch {
    uint32_t ntx, nstates;
    const uint32_t *key;          // nstates * 8
    const uint32_t *begin;        // ntx + 1
    const uint32_t *id;           // ntx * 8
    const uint32_t *caller;       // ntx
    const uint8_t *enable;        // ntx, or null = all
    uint32_t *btab, bmask;        // batch-local table of state indices, bmask + 1 slots
    uint32_t *rep, *res, *state_tx, *owner, *last;   // nstates each
    uint8_t *tx_status, *state_conflict;
    uint32_t *cons_id, *cons_index, *cons_caller;
    uint32_t *dstat;              // CVU_D_WORDS
};

// The slot holding `key`, or CVU_NONE.  Read-only.
CV_HD uint32_t cvu_find(const CvUniqTable &T, const uint32_t *key, uint64_t h, uint32_t *dstat) {
    const uint32_t *keys = T.key;
    // the set counts wraps into CVU_D_WRAPS beside max-probe and error; the tag is compared before the key
    return cvt_find(T.occ, T.mask, [keys](uint32_t slot) { return keys + 8 * (size_t)slot; }, key, h, dstat,
                    dstat + CVU_D_WRAPS);
}

// Puts a key that is absent and that no other lane inserts: the first slot this lane's CAS turns from empty.
CV_HD void cvu_insert(const CvUniqTable &T, const uint32_t *key, const uint32_t *id, uint32_t index, uint32_t caller,
                      uint32_t *dstat) {
    // counts wraps into CVU_D_WRAPS as cvu_find does; an overflow sets CVU_D_ERROR and stores nothing
    const CvWalk<uint32_t> w = cvt_claim(T.occ, T.mask, cvu_hash(key, T.seed), dstat + CVU_D_WRAPS);
    if (w.stopped) {
        cvu_copy8(T.key + 8 * (size_t)w.slot, key);
        cvu_copy8(T.id + 8 * (size_t)w.slot, id);
        T.index[w.slot] = index;
        T.caller[w.slot] = caller;
    }
    cvt_note(dstat, w);
}

// growth: one lane per slot of the old table re-inserts its record into the new one
CV_HD void cvu_rehash(const CvUniqTable &from, const CvUniqTable &to, uint32_t slot, uint32_t *dstat) {
    if (from.occ[slot] == 0) return;
    cvu_insert(to, from.key + 8 * (size_t)slot, from.id + 8 * (size_t)slot, from.index[slot], from.caller[slot], dstat);
}

// cv_uniq_lookup, one lane per key
CV_HD void cvu_lookup(const CvUniqTable &T, const uint32_t *key, uint32_t i, uint8_t *found, uint32_t *cons_id,
                      uint32_t *cons_index, uint32_t *cons_caller, uint32_t *dstat) {
    const uint32_t *k = key + 8 * (size_t)i;
    const uint32_t s = cvu_find(T, k, cvu_hash(k, T.seed), dstat);
    found[i] = s != CVU_NONE;
    if (s == CVU_NONE) return;
    cvu_copy8(cons_id + 8 * (size_t)i, T.id + 8 * (size_t)s);
    cons_index[i] = T.index[s];
    cons_caller[i] = T.caller[s];
}

// ---- commit_batch, in the order of the header comment
CV_HD void cvu_init(const CvUniqBatch &B, uint32_t *stat, uint32_t t) {
    stat[t] = (B.enable && !B.enable[t]) ? CVU_REJECTED : CVU_UNDECIDED;
    for (uint32_t i = B.begin[t]; i < B.begin[t + 1]; i++) B.state_tx[i] = t;
}

// stat == null: cv_uniq_load's check (no requests; the caller reads rep and res)
CV_HD void cvu_group(const CvUniqTable &T, const CvUniqBatch &B, uint32_t *stat, uint32_t i) {
    const uint32_t *k = B.key + 8 * (size_t)i;
    const uint64_t h = cvu_hash(k, T.seed);
    uint32_t rep = CVU_NONE;
    // from bits 20.. of the resident find's h; a plain CAS, ANY winner is the representative; no wraps, no max-probe
    cv_walk(B.bmask, (uint32_t)(h >> 20), nullptr, [&](uint32_t slot) {
        const uint32_t old = cvu_atomic_cas(B.btab + slot, CVU_NONE, i);
        if (old == CVU_NONE)
            rep = i;
        else if (cvu_key_eq(B.key + 8 * (size_t)old, k))
            rep = old;
        return rep != CVU_NONE;
    });
    if (rep == CVU_NONE) {                      // more states than slots: the caller sized the table at twice the states
        B.dstat[CVU_D_ERROR] = 1;
        rep = i;
    }
    B.rep[i] = rep;
    const uint32_t r = cvu_find(T, k, h, B.dstat);
    B.res[i] = r;
    if (r != CVU_NONE && stat) stat[B.state_tx[i]] = CVU_REJECTED;
}

CV_HD void cvu_claim(const CvUniqBatch &B, const uint32_t *stat, uint32_t t) {
    if (stat[t] == CVU_REJECTED) return;
    for (uint32_t i = B.begin[t]; i < B.begin[t + 1]; i++) cvu_atomic_min(B.owner + B.rep[i], t);
}

// returns 1 while the request stays undecided
CV_HD uint32_t cvu_decide(const CvUniqBatch &B, const uint32_t *stat_in, uint32_t *stat_out, uint32_t t) {
    uint32_t st = stat_in[t];
    if (st == CVU_UNDECIDED) {
        bool all = true, hit = false;
        for (uint32_t i = B.begin[t]; i < B.begin[t + 1]; i++) {
            const uint32_t o = B.owner[B.rep[i]];
            if (o != t) {
                all = false;
                if (o < t && stat_in[o] == CVU_ACCEPTED) hit = true;
            }
        }
        st = all ? CVU_ACCEPTED : hit ? CVU_REJECTED : CVU_UNDECIDED;
    }
    stat_out[t] = st;
    return st == CVU_UNDECIDED;
}

CV_HD void cvu_take(const CvUniqBatch &B, uint32_t t) {
    const uint32_t b = B.begin[t];
    for (uint32_t i = b; i < B.begin[t + 1]; i++) {
        const uint32_t r = B.rep[i];
        B.owner[r] = t;
        B.last[r] = i - b;
    }
}

CV_HD void cvu_own(const CvUniqBatch &B, const uint32_t *stat, uint32_t t) {
    if (stat[t] == CVU_ACCEPTED) cvu_take(B, t);
}

// the serial tail's step for request t; ONE lane calls it for the undecided requests in ascending order
CV_HD void cvu_tail_one(const CvUniqBatch &B, uint32_t *stat, uint32_t t) {
    bool hit = false;
    for (uint32_t i = B.begin[t]; i < B.begin[t + 1]; i++) {
        const uint32_t o = B.owner[B.rep[i]];
        if (o != CVU_NONE && o != t) hit = true;
    }
    stat[t] = hit ? CVU_REJECTED : CVU_ACCEPTED;
    if (!hit) cvu_take(B, t);
    B.dstat[CVU_D_TAIL] += 1;
}

// returns the records the request inserted
CV_HD uint32_t cvu_report(const CvUniqTable &T, const CvUniqBatch &B, const uint32_t *stat, uint32_t t) {
    const uint32_t b = B.begin[t], e = B.begin[t + 1];
    if (B.enable && !B.enable[t]) {
        B.tx_status[t] = CVU_SKIPPED;
        for (uint32_t i = b; i < e; i++) B.state_conflict[i] = 0;
        return 0;
    }
    if (stat[t] == CVU_ACCEPTED) {
        B.tx_status[t] = CVU_OK;
        uint32_t put = 0;
        for (uint32_t i = b; i < e; i++) {
            B.state_conflict[i] = 0;
            if (B.last[B.rep[i]] != i - b) continue;          // an earlier copy of a key the request repeats
            cvu_insert(T, B.key + 8 * (size_t)i, B.id + 8 * (size_t)t, i - b, B.caller[t], B.dstat);
            put++;
        }
        return put;
    }
    if (stat[t] != CVU_REJECTED) B.dstat[CVU_D_ERROR] = 1;    // the tail leaves nothing undecided
    B.tx_status[t] = CVU_CONFLICT;
    for (uint32_t i = b; i < e; i++) {
        const uint32_t r = B.res[i], rp = B.rep[i], o = B.owner[rp];
        uint8_t c = 0;
        if (r != CVU_NONE) {
            c = 1;
            cvu_copy8(B.cons_id + 8 * (size_t)i, T.id + 8 * (size_t)r);
            B.cons_index[i] = T.index[r];
            B.cons_caller[i] = T.caller[r];
        } else if (o < t) {
            c = 1;
            cvu_copy8(B.cons_id + 8 * (size_t)i, B.id + 8 * (size_t)o);
            B.cons_index[i] = B.last[rp];
            B.cons_caller[i] = B.caller[o];
        }
        B.state_conflict[i] = c;
    }
    return 0;
}

// ---- cv_uniq_load: cvu_group with stat == null over the n keys, then per key
CV_HD void cvu_load_check(const CvUniqBatch &B, uint32_t i) {
    if (B.rep[i] != i || B.res[i] != CVU_NONE) B.dstat[CVU_D_BAD] = 1;
}
CV_HD void cvu_load_put(const CvUniqTable &T, const CvUniqBatch &B, uint32_t i) {
    cvu_insert(T, B.key + 8 * (size_t)i, B.id + 8 * (size_t)i, B.cons_index[i], B.caller[i], B.dstat);
}

// ---- snapshot: the per-lane pieces of count and emit (the header comment); the scan between them is the caller's
CV_HD uint32_t cvu_snap_occupied(const CvUniqTable &T, const CvUniqSnap &S, uint32_t i) {
    return i < S.slot_end - S.slot_begin && T.occ[S.slot_begin + i] != 0;
}
// lane i of the window holds an occupied slot, the rank-th of the window
CV_HD void cvu_snap_emit(const CvUniqTable &T, const CvUniqSnap &S, uint32_t i, uint32_t rank) {
    const uint32_t slot = S.slot_begin + i;
    if (rank < S.max_entries) {
        cvu_copy8_aligned(S.key + 8 * (size_t)rank, T.key + 8 * (size_t)slot);
        cvu_copy8_aligned(S.id + 8 * (size_t)rank, T.id + 8 * (size_t)slot);
        S.index[rank] = T.index[slot];
        S.caller[rank] = T.caller[slot];
    } else if (rank == S.max_entries) {
        S.out[CVU_SNAP_NEXT] = slot;
    }
}
// ONE lane, after the scan wrote the total
CV_HD void cvu_snap_close(const CvUniqSnap &S) {
    const uint32_t total = S.out[CVU_SNAP_TOTAL];
    S.out[CVU_SNAP_COUNT] = total < S.max_entries ? total : S.max_entries;
    if (total <= S.max_entries) S.out[CVU_SNAP_NEXT] = S.slot_end;
}
