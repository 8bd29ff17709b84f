// cv_tearoff.h — the decisions between the stages of cv_filtered_verify and cv_tearoff_sign_batch: the verifier side
// of a tear-off, FilteredTransaction.verify (core/src/main/kotlin/net/corda/core/transactions/MerkleTransaction.kt:
// 112-117,173-178) and the oracle's NodeInterestRates.Oracle.sign (samples/irs-demo/src/main/kotlin/net/corda/irs/api/
// NodeInterestRates.kt:190-225), for a whole batch.  The per-lane core of cv_k_tearoff.hip; __host__ __device__, so
// tests/tearoff_harness.cpp runs the lanes on the CPU one after another, in any order.
//
// THREE STEPS, one lane per filtered leaf or per tear-off, no lane reading what another lane of its kernel writes:
//   check     per filtered leaf: FilteredLeaves.getFilteredHashes (MerkleTransaction.kt:112-117) — the SHA-256 digest
//             of the leaf blob, as the leaf kernel left it (big-endian state words), becomes the 32 digest bytes
//             cv_pmt_verify (cv_verify.h) loads as a check hash.  The check list of tear-off t is the digests of its
//             leaves [tx_leaf_begin[t], tx_leaf_begin[t + 1]), so tx_leaf_begin is the verify's check_begin.
//   gate      per tear-off: the outcome, first match wins in the reference's order —
//               NO_LEAVES       `hashes.size == 0` (MerkleTransaction.kt:175-176) is tested before the tree is touched,
//                               so it wins over a malformed encoding
//               MALFORMED       the nodes are not a tree encoding (no reference counterpart: a PartialTree object cannot
//                               be one)
//               VERIFY_FAILED   "Couldn't verify partial Merkle tree." (NodeInterestRates.kt:191-193)
//               NOT_COMMANDS    the require at :197: some leaf is an input, an output or an attachment
//               WRONG_COMMAND   :199-205: some command is not a Fix this oracle signs
//               UNKNOWN         :213-217: the first fix, in order, that the oracle does not know as given
//             from the leaf count, the verify's verdict and status and the service's byte per leaf (leaf_pre).  Among
//             the last three the LOWEST class present decides (each of the reference's tests looks at all leaves before
//             the next one runs), first_bad = the first leaf of that class.  The reference's `fixes.isEmpty()` branch
//             (:208-209) cannot be reached here: past the first two tests there is at least one leaf and every leaf is
//             a command the oracle vouches for, so `fixes` has as many entries as there are leaves.
//             The gate also restates the verify's results under FilteredTransaction.verify's rule (fv_verdict,
//             fv_status: CVT_PMT_NO_INCLUDED for no leaves), which is all cv_filtered_verify returns.
//   place     accepted tear-off t at position pos of the signing records: list[pos] = t, off = 32 t, len = 32 over the
//             device copy of the roots (the ordered compaction: a block scan in the kernel, a running count in the
//             harness).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef CV_HD
#define CV_HD __host__ __device__ __forceinline__
#endif

// outcome[t] (include/cordaverify.h CV_TS_*)
#define CVT_SUCCESS 0
#define CVT_NO_LEAVES 1
#define CVT_MALFORMED 2
#define CVT_VERIFY_FAILED 3
#define CVT_NOT_COMMANDS 4
#define CVT_WRONG_COMMAND 5
#define CVT_UNKNOWN 6
#define CVT_NO_LEAF 0xffffffffu
// leaf_pre: the service's verdict on a filtered leaf's content (0 = fine)
#define CVT_PRE_NOT_COMMAND 1
#define CVT_PRE_WRONG_COMMAND 2
#define CVT_PRE_UNKNOWN 3
// the verify's statuses (include/cordaverify.h CV_PMT_*)
#define CVT_PMT_OK 0
#define CVT_PMT_MALFORMED 2
#define CVT_PMT_NO_INCLUDED 4
// threads of the compaction kernel's one workgroup: the scan walks the batch in chunks of this many tear-offs
#define CVT_SCAN_BLOCK 1024

struct CvTearoff {
    uint32_t ntx, nleaves;
    // check
    const uint32_t *leaf_digest;       // nleaves * 8: the leaf kernel's digests, big-endian state words
    uint32_t *check;                   // nleaves * 8: the words of the 32 digest bytes
    // gate
    const uint32_t *tx_leaf_begin;     // ntx + 1
    const uint8_t *verdict, *status;   // ntx each: cv_pmt_verify's
    const uint8_t *leaf_pre;           // nleaves, or null = none
    uint8_t *fv_verdict, *fv_status;   // ntx each, or null: FilteredTransaction.verify's results
    uint8_t *outcome;                  // ntx
    uint32_t *first_bad;               // ntx
    // place
    uint32_t *list;                    // ntx: accepted tear-offs, ascending
    uint64_t *sign_off;                // ntx
    uint32_t *sign_len;                // ntx
};

CV_HD uint32_t cvt_bswap32(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}

CV_HD void cvt_check(const CvTearoff &T, uint32_t i) {
    const uint32_t *d = T.leaf_digest + (size_t)i * 8;
    uint32_t *c = T.check + (size_t)i * 8;
    for (int q = 0; q < 8; q++) c[q] = cvt_bswap32(d[q]);
}

CV_HD void cvt_gate(const CvTearoff &T, uint32_t t) {
    const uint32_t b = T.tx_leaf_begin[t], e = T.tx_leaf_begin[t + 1];
    uint32_t out = CVT_SUCCESS, bad = CVT_NO_LEAF, v = 0, st = CVT_PMT_OK;
    if (e == b) {
        out = CVT_NO_LEAVES;
        st = CVT_PMT_NO_INCLUDED;
    } else if (T.status[t] != CVT_PMT_OK) {
        out = CVT_MALFORMED;
        st = T.status[t];
    } else if (!T.verdict[t]) {
        out = CVT_VERIFY_FAILED;
    } else {
        v = 1;
        if (T.leaf_pre) {
            // the first leaf of each class; the lowest class present decides
            uint32_t f1 = CVT_NO_LEAF, f2 = CVT_NO_LEAF, f3 = CVT_NO_LEAF;
            for (uint32_t i = e; i-- > b;) {
                const uint32_t p = T.leaf_pre[i];
                f1 = p == CVT_PRE_NOT_COMMAND ? i : f1;
                f2 = p == CVT_PRE_WRONG_COMMAND ? i : f2;
                f3 = p == CVT_PRE_UNKNOWN ? i : f3;
            }
            if (f1 != CVT_NO_LEAF)
                out = CVT_NOT_COMMANDS, bad = f1;
            else if (f2 != CVT_NO_LEAF)
                out = CVT_WRONG_COMMAND, bad = f2;
            else if (f3 != CVT_NO_LEAF)
                out = CVT_UNKNOWN, bad = f3;
        }
    }
    if (T.fv_verdict) T.fv_verdict[t] = (uint8_t)v;
    if (T.fv_status) T.fv_status[t] = (uint8_t)st;
    T.outcome[t] = (uint8_t)out;
    T.first_bad[t] = bad;
}

// 1 when tear-off t was accepted (its root is to be signed)
CV_HD uint32_t cvt_accepted(const CvTearoff &T, uint32_t t) { return T.outcome[t] == CVT_SUCCESS ? 1u : 0u; }

// accepted tear-off t takes position pos of the signing records
CV_HD void cvt_place(const CvTearoff &T, uint32_t t, uint32_t pos) {
    T.list[pos] = t;
    T.sign_off[pos] = (uint64_t)t * 32;
    T.sign_len[pos] = 32;
}
