// cv_keystore.h — the node's key management service on the device: KeyManagementService (core/src/main/kotlin/net/
// corda/core/node/services/Services.kt:189-219) as PersistentKeyManagementService / E2ETestKeyManagementService keep it
// (node/.../keys/PersistentKeyManagementService.kt:40-66: a map PublicKey -> PrivateKey, freshKey() = generateKeyPair()
// + keys[public] = private, toPrivate(pk) = keys[pk] ?: throw IllegalStateException) and the builder's signing step
// over it (TransactionBuilder.signWith, core/.../transactions/TransactionBuilder.kt:93-98, driven by the flows' loops:
// CashFlow.kt:39-47, TwoPartyTradeFlow.kt:227-235).  The per-lane core of cv_k_keystore.hip; __host__ __device__, so
// tests/keystore_harness.cpp runs the lanes on the CPU one after another, in any order (the atomics reduce to plain
// operations there).
//
// THE STORE (CvKeyTable): a table of cv_table.h (probing, sizing and hashing are described there) with a per-store
// random seed and a floor of 16 slots.  occ (0 = empty, else the tag: a 32-bit fingerprint of the key's hash with bit
// 0 set) and, per slot, the expanded record a | prefix | Abyte (24 words: the 96 bytes of a cv_signer record).  Abyte,
// the encoded public key, is what the slot is found by: the identity of a key is its 32 encoded bytes (a counterparty
// can grind the keys it asks a node to sign with, as it can state keys).
//
// ONE add (n seeds), a kernel per step:
//   expand    per seed i: cv_key_expand -> the staged record i and pk[i]                        (cv_k_keystore.hip)
//   group     per record i: cvd_insert into a call-local table of record INDICES (cv_keydedupe.h): a key's slot ends
//             at its FIRST occurrence in index order, whichever lane won
//   classify  per record i, the call-local table read-only by then: first[i] (cvd_mark) and a read-only probe of the
//             store -> status[i] = ADDED iff i is its key's first occurrence and the key is not resident
//   put       per ADDED record: the keys put by one call are distinct and absent, so the insert claims the first
//             slot whose atomicCAS(occ, 0, tag) succeeds, without a key compare, and writes the record with plain
//             stores; the kernel boundary publishes it (no lane of this kernel reads a slot that was empty before it)
// THE RESULT IS A FUNCTION OF THE INPUT BYTES ALONE (which slot a key lands in depends on the lanes' order; the
// statuses, the keys and what every later lookup of a key finds do not).
//
// SIGNING reads the store only: lookup (per record: the slot of its key, or none) and then the signing kernel, whose
// lanes read their slot's record where they consume it.  The builder's step for a batch of transactions (cks_tx_gate,
// one lane per transaction) walks the transaction's keys in order as the flows' loops do; the first index j at which
// something fails settles the status and first_bad:
//   NO_KEY          key j is not in the store (CashFlow.kt:43 / Services.kt:210, thrown before signWith)
//   ALREADY_SIGNED  key j equals an earlier key of the transaction (TransactionBuilder.kt:94's check); the scan of the
//                   earlier keys is per lane and quadratic in ONE transaction's signer count
//   EMPTY           no leaves: toWireTransaction().id raises inside the first signWith, so at j = 0 after the first
//                   two checks; a transaction with no leaves and no keys is EMPTY too (toSignedTransaction, :139-140),
//                   with first_bad = 0
// and a transaction that is not OK has every slot of its keys set to none, so its lanes leave the signing kernel
// before they read a key record and its signatures are zero.
//
// NO LANE WAITS FOR ANOTHER LANE: no spin, lock or flag.  EVERY PROBE IS BOUNDED: each is cv_walk (cv_table.h), which
// looks at no more than its table's slot count, and sets dstat[CKS_D_ERROR] when it runs out (the host returns
// CV_E_HIP); the capacity check rules it out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cv_keydedupe.h"

#define CKS_NONE CVT_NONE          // no slot: the key is absent, or its transaction is abandoned
#define CKS_REC_WORDS 24           // a | prefix | Abyte
#define CKS_REC_A 0
#define CKS_REC_PREFIX 8
#define CKS_REC_ABYTE 16
// status bytes (include/cordaverify.h CV_KS_*, CV_ST_*)
#define CKS_ADDED 0
#define CKS_PRESENT 1
#define CKS_OK 0
#define CKS_NO_KEY 1
#define CKS_ST_OK 0
#define CKS_ST_NO_KEY 1
#define CKS_ST_ALREADY_SIGNED 2
#define CKS_ST_EMPTY 3
// words of the per-call device counters
#define CKS_D_ERROR CVT_D_ERROR     // a probe ran out of slots
#define CKS_D_MAXPROBE CVT_D_MAXPROBE   // longest probe of the store (slots looked at)
#define CKS_D_ADDED 2              // records the call put
#define CKS_D_WORDS 4

struct CvKeyTable {
    uint32_t *occ;                 // mask + 1 tags
    uint32_t *rec;                 // (mask + 1) * CKS_REC_WORDS
    uint32_t mask;                 // slots - 1
    uint64_t seed;
};
#ifndef __HIP_DEVICE_COMPILE__
// the table in ONE allocation of CKS_SLOT_BYTES * slots at base: occ | rec (16-byte aligned: slots >= 16)
#define CKS_SLOT_BYTES (4 * (1 + CKS_REC_WORDS))
inline CvKeyTable cks_carve(void *base, size_t slots, uint64_t seed) {
    uint32_t *p = static_cast<uint32_t *>(base);
    return CvKeyTable{p, p + slots, (uint32_t)(slots - 1), seed};
}
#endif

// the builder's signing step: ntx transactions, transaction t signed by keys [sig_begin[t], sig_begin[t + 1])
struct CvKeyTx {
    uint32_t ntx;
    const uint32_t *leaf_begin;    // ntx + 1
    const uint32_t *sig_begin;     // ntx + 1
    const uint32_t *pk;            // nsig * 8
    uint32_t *slot;                // nsig: the key's slot, CKS_NONE for every key of a transaction that is not OK
    uint64_t *off;                 // nsig: 32 t, the transaction's id among the ids
    uint32_t *len;                 // nsig: 32
    uint8_t *tx_status;            // ntx
    uint32_t *first_bad;           // ntx
    uint32_t *dstat;               // CKS_D_WORDS
};

// The slot holding `key`, or CKS_NONE.  Read-only.
CV_HD uint32_t cks_find(const CvKeyTable &T, const uint32_t *key, uint32_t *dstat) {
    const uint32_t *rec = T.rec;
    // the store counts NO wraps (word 2 of its counters is CKS_D_ADDED); max-probe and error as the set's
    return cvt_find(
        T.occ, T.mask, [rec](uint32_t slot) { return rec + CKS_REC_WORDS * (size_t)slot + CKS_REC_ABYTE; }, key,
        cvu_hash(key, T.seed), dstat, nullptr);
}

// Puts a record whose key is absent and that no other lane inserts: the first slot this lane's CAS turns from empty.
CV_HD void cks_insert(const CvKeyTable &T, const uint32_t *rec, uint32_t *dstat) {
    // no wraps counted, as cks_find; an overflow sets CKS_D_ERROR and stores nothing
    const CvWalk<uint32_t> w = cvt_claim(T.occ, T.mask, cvu_hash(rec + CKS_REC_ABYTE, T.seed), nullptr);
    if (w.stopped) {
        uint32_t *d = T.rec + CKS_REC_WORDS * (size_t)w.slot;
#pragma unroll
        for (int q = 0; q < CKS_REC_WORDS; q++) d[q] = rec[q];
    }
    cvt_note(dstat, w);
}

// growth: one lane per slot of the old table re-inserts its record into the new one
CV_HD void cks_rehash(const CvKeyTable &from, const CvKeyTable &to, uint32_t slot, uint32_t *dstat) {
    if (from.occ[slot] == 0) return;
    cks_insert(to, from.rec + CKS_REC_WORDS * (size_t)slot, dstat);
}

// add, after cvd_insert over every record of D (D.pk: the records' public keys): first occurrence and residency
CV_HD void cks_classify(const CvKeyTable &T, const CvDedupe &D, uint32_t i, uint8_t *status, uint32_t *dstat) {
    cvd_mark(D, i);
    const bool resident = cks_find(T, D.pk + 8 * (size_t)i, dstat) != CKS_NONE;
    status[i] = (D.first[i] == i && !resident) ? CKS_ADDED : CKS_PRESENT;
}

// add, last step: rec = the staged records (n * CKS_REC_WORDS)
CV_HD void cks_put(const CvKeyTable &T, const CvDedupe &D, uint32_t i, const uint32_t *rec, const uint8_t *status,
                   uint32_t *dstat) {
    if (i == 0 && D.stat[CVD_STAT_OK] != CVD_NONE) dstat[CKS_D_ERROR] = 1;   // the call-local table ran out of slots
    if (status[i] != CKS_ADDED) return;
    cks_insert(T, rec + CKS_REC_WORDS * (size_t)i, dstat);
    cvu_atomic_add(dstat + CKS_D_ADDED, 1);
}

// contains / the lookup ahead of signing: slot (optional) = the key's slot or CKS_NONE; flag (optional) = `present`
// for a resident key, else 1 - present (found: present = 1; a signing status: present = CKS_OK)
CV_HD void cks_lookup(const CvKeyTable &T, const uint32_t *pk, uint32_t i, uint32_t *slot, uint8_t *flag, uint8_t present,
                      uint32_t *dstat) {
    const uint32_t s = cks_find(T, pk + 8 * (size_t)i, dstat);
    if (slot) slot[i] = s;
    if (flag) flag[i] = s != CKS_NONE ? present : (uint8_t)(1 - present);
}

// the builder's signing step for transaction t (the header comment)
CV_HD void cks_tx_gate(const CvKeyTable &T, const CvKeyTx &X, uint32_t t) {
    const uint32_t sb = X.sig_begin[t], se = X.sig_begin[t + 1];
    const bool empty = X.leaf_begin[t + 1] == X.leaf_begin[t];
    uint32_t st = CKS_ST_OK, bad = CKS_NONE;
    for (uint32_t j = sb; j < se && st == CKS_ST_OK; j++) {
        const uint32_t *k = X.pk + 8 * (size_t)j;
        const uint32_t s = cks_find(T, k, X.dstat);
        X.slot[j] = s;
        if (s == CKS_NONE) {
            st = CKS_ST_NO_KEY;
        } else {
            for (uint32_t i = sb; i < j; i++)
                if (cvu_key_eq(X.pk + 8 * (size_t)i, k)) st = CKS_ST_ALREADY_SIGNED;
            if (st == CKS_ST_OK && empty) st = CKS_ST_EMPTY;   // only j == sb gets here with an empty transaction
        }
        if (st != CKS_ST_OK) bad = j - sb;
    }
    if (st == CKS_ST_OK && empty) {             // no keys: toSignedTransaction computes the id
        st = CKS_ST_EMPTY;
        bad = 0;
    }
    for (uint32_t j = sb; j < se; j++) {
        if (st != CKS_ST_OK) X.slot[j] = CKS_NONE;
        X.off[j] = 32ull * t;
        X.len[j] = 32;
    }
    X.tx_status[t] = (uint8_t)st;
    X.first_bad[t] = bad;
}
