// cv_notary.h — the decisions between the stages of cv_notarise_batch: NotaryFlow.Service.call (core/src/main/kotlin/
// net/corda/flows/NotaryFlow.kt:96-146) with ValidatingNotaryFlow.beforeCommit (ValidatingNotaryFlow.kt:24-45) for a
// whole batch.  The per-lane core of cv_k_notary.hip; __host__ __device__, so tests/notary_harness.cpp runs the lanes
// on the CPU one after another, in any order.
//
// THREE STEPS, one lane per transaction or per state, no lane reading what another lane of its kernel writes:
//   gate      per transaction: the outcome BEFORE the commit, first match wins in the reference's order —
//               EMPTY, ID_MISMATCH   `val wtx = stx.tx` (NotaryFlow.kt:99; SignedTransaction.kt:34-38) sits outside the try
//               TIMESTAMP_INVALID    validateTimestamp (NotaryFlow.kt:102,115-119): the host's TimestampChecker, tx_pre
//               TX_INVALID, BAD_KEY  checkSignaturesAreValid (SignedTransaction.kt:82-87) stops at the FIRST signature
//                                    that fails: its exception settles the class (ValidatingNotaryFlow.kt:31-35); no
//                                    signatures at all is TX_INVALID by the rule of cv_tx_verdicts
//               MALFORMED, SIGNATURES_MISSING   the missing-signers status (cv_ck.h) of the same batch
//             and enable[t] = 1 iff none matched: the byte array the uniqueness kernels consume.
//   gather    per state: the SHA-256 digest of its input leaf, as the leaf kernel left it (big-endian state words),
//             byte-swapped into the words of the byte string that CvUniqBatch::key holds.  It runs BETWEEN the leaf
//             kernel and the tree kernel: the tree folds the digests in place.
//   finalise  per transaction: outcome = the gate's, or CONFLICT / SUCCESS from the uniqueness status; the accepted
//             transactions are listed in ascending order (a block scan in the kernel, a running count in the harness)
//             as the signing kernel's records: list[j] = t, off[j] = 32 t, len[j] = 32 over the device ids.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef CV_HD
#define CV_HD __host__ __device__ __forceinline__
#endif

// outcome[t] (include/cordaverify.h CV_NS_*)
#define CVN_SUCCESS 0
#define CVN_EMPTY 1
#define CVN_ID_MISMATCH 2
#define CVN_TIMESTAMP_INVALID 3
#define CVN_TX_INVALID 4
#define CVN_BAD_KEY 5
#define CVN_SIGNATURES_MISSING 6
#define CVN_MALFORMED 7
#define CVN_CONFLICT 8
#define CVN_NO_SIG 0xffffffffu
// sig_pre: what the host's prefilter found before the call
#define CVN_PRE_SIGNATURE 1        // SignatureException (a signature that is not 64 bytes)
#define CVN_PRE_KEY 2              // InvalidKeyException (a key that is not EdDSA)
// the statuses the gate and finalise read (cv_ck.h CVCK_VS_*, cv_uniq.h CVU_*, CV_SIG_BAD_KEY)
#define CVN_VS_MISSING 2
#define CVN_VS_MALFORMED 3
#define CVN_UNIQ_CONFLICT 1
#define CVN_SIG_BAD_KEY 1
// the word of the uniqueness set's per-call counters (cv_uniq.h CVU_D_*; 6 and 7 are free there) that takes the
// number of accepted transactions, so it comes back with the counters' read-back
#define CVN_D_ACCEPTED 6
// threads of the finalise kernel's one workgroup: the scan walks the batch in chunks of this many transactions
#define CVN_SCAN_BLOCK 1024

struct CvNotary {
    uint32_t ntx, nstates;
    int validating;
    const uint8_t *mstatus;            // ntx: the Merkle status (non-zero = no leaves)
    const uint32_t *id, *claimed;      // ntx * 8: the words of the recomputed and the claimed id bytes
    const uint8_t *tx_pre;             // ntx, or null = none
    // validating only
    const uint32_t *tx_sig_begin;      // ntx + 1
    const uint64_t *bitmap;            // the verify's verdict bits
    const uint8_t *sig_status;         // nsig: CV_SIG_*
    const uint8_t *sig_pre;            // nsig, or null = none
    const uint8_t *ck_status;          // ntx: CV_VS_*
    // gate -> uniqueness kernels, finalise
    uint8_t *pre, *enable;             // ntx each
    uint32_t *first_bad;               // ntx
    // gather
    const uint32_t *leaf_digest;       // the leaf kernel's digests, 8 big-endian state words a leaf
    const uint32_t *state_leaf;        // nstates: the leaf index of each state
    uint32_t *key;                     // nstates * 8
    // finalise
    const uint8_t *uniq_status;        // ntx: CV_UNIQ_*
    uint8_t *outcome;                  // ntx
    uint32_t *list;                    // ntx: accepted transactions, ascending
    uint64_t *sign_off;                // ntx
    uint32_t *sign_len;                // ntx
};

CV_HD uint32_t cvn_bswap32(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}

// The first signature of [b, e), in order, that fails: a sig_pre flag or a zero verdict bit.  CVN_NO_SIG if none.
// The bitmap is read a word at a time, so a range that straddles words costs one load per word it touches.
CV_HD uint32_t cvn_first_bad(const CvNotary &N, uint32_t b, uint32_t e) {
    uint32_t i = b;
    while (i < e) {
        const uint32_t w = i >> 6, stop = (w + 1) << 6 < e ? (w + 1) << 6 : e;
        const uint64_t word = N.bitmap[w];
        for (; i < stop; i++)
            if (!((word >> (i & 63)) & 1) || (N.sig_pre && N.sig_pre[i])) return i;
    }
    return CVN_NO_SIG;
}

CV_HD void cvn_gate(const CvNotary &N, uint32_t t) {
    uint32_t out = CVN_SUCCESS, bad = CVN_NO_SIG;
    if (N.mstatus[t])
        out = CVN_EMPTY;
    else {
        uint32_t diff = 0;
        for (int q = 0; q < 8; q++) diff |= N.id[(size_t)t * 8 + q] ^ N.claimed[(size_t)t * 8 + q];
        if (diff)
            out = CVN_ID_MISMATCH;
        else if (N.tx_pre && N.tx_pre[t])
            out = CVN_TIMESTAMP_INVALID;
        else if (N.validating) {
            const uint32_t b = N.tx_sig_begin[t], e = N.tx_sig_begin[t + 1];
            bad = cvn_first_bad(N, b, e);
            if (bad != CVN_NO_SIG) {
                // the host's prefilter ran before the engine would have seen the record: its class comes first
                const uint32_t p = N.sig_pre ? N.sig_pre[bad] : 0;
                out = p == CVN_PRE_KEY || (p == 0 && N.sig_status[bad] == CVN_SIG_BAD_KEY) ? CVN_BAD_KEY : CVN_TX_INVALID;
            } else if (e == b)
                out = CVN_TX_INVALID;
            else if (N.ck_status[t] == CVN_VS_MALFORMED)
                out = CVN_MALFORMED;
            else if (N.ck_status[t] == CVN_VS_MISSING)
                out = CVN_SIGNATURES_MISSING;
        }
    }
    N.pre[t] = (uint8_t)out;
    N.enable[t] = out == CVN_SUCCESS ? 1 : 0;
    N.first_bad[t] = bad;
}

CV_HD void cvn_gather(const CvNotary &N, uint32_t i) {
    const uint32_t *d = N.leaf_digest + (size_t)N.state_leaf[i] * 8;
    uint32_t *k = N.key + (size_t)i * 8;
    for (int q = 0; q < 8; q++) k[q] = cvn_bswap32(d[q]);
}

// the outcome of transaction t; returns 1 when it was committed (its id is to be signed)
CV_HD uint32_t cvn_final(const CvNotary &N, uint32_t t) {
    uint32_t out = N.pre[t];
    if (out == CVN_SUCCESS && N.uniq_status[t] == CVN_UNIQ_CONFLICT) out = CVN_CONFLICT;
    N.outcome[t] = (uint8_t)out;
    return out == CVN_SUCCESS ? 1u : 0u;
}

// accepted transaction t takes position pos of the signing records
CV_HD void cvn_place(const CvNotary &N, uint32_t t, uint32_t pos) {
    N.list[pos] = t;
    N.sign_off[pos] = (uint64_t)t * 32;
    N.sign_len[pos] = 32;
}
