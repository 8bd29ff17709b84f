// cv_ck.h — missing signers of a batch: SignedTransaction.getMissingSignatures (core/src/main/kotlin/net/corda/core/
// transactions/SignedTransaction.kt:89-93, `tx.mustSign.filter { !it.isFulfilledBy(sigKeys) }`) over weighted-threshold
// CompositeKey trees (core/.../crypto/CompositeKey.kt:22-108: Leaf.isFulfilledBy :49, Node.isFulfilledBy :75-81), and
// the verdict verifySignatures draws from it (SignedTransaction.kt:58-72).  The per-lane core of cv_k_ck.hip;
// __host__ __device__, so tests/ck_harness.cpp runs the lanes on the CPU one after another, in any order.
//
// ENCODING (include/cordaverify.h, cv_missing_signers): every mustSign entry (a requirement) flattened in post-order,
// its root last; node k has kind[k], a Leaf its 32 key bytes leaf_key[k], a Node threshold[k] and the children
// child[child_begin[k] .. child_begin[k + 1]) with weight[] beside them — absolute node indices inside the same
// requirement and below k, so nodes evaluate in index order without recursion or a stack, and a node shared by several
// parents (a DAG) evaluates as the tree it unfolds to.  Requirement r = nodes [req_begin[r], req_begin[r + 1]);
// transaction t = requirements [tx_req_begin[t], tx_req_begin[t + 1]) and signer keys [tx_sig_begin[t], tx_sig_begin[t + 1]).
//
// SEMANTICS, the reference's: a Leaf is fulfilled iff its key is among the transaction's signer keys (all 32 bytes
// compared, nothing decoded); a Node iff the sum of the weights of its fulfilled children, a Kotlin Int that WRAPS, is
// >= its threshold as signed 32-bit numbers.  The sum is kept unsigned and reinterpreted (signed overflow is undefined
// in C++).  A child listed twice counts twice; a Node without children is fulfilled iff threshold <= 0.
//
// TRUST: the three outer range arrays (req_begin, tx_req_begin, tx_sig_begin) are the caller's word (the host form
// checks them before any device work); everything per node is checked here — a kind outside {0, 1}, a child range that
// descends or ends past nchild, a child outside [req_begin[r], k), an empty requirement make the requirement MALFORMED
// (req_missing 2) and its transaction CV_VS_MALFORMED.  A lane never reads outside its requirement's nodes, the child
// entries of a checked range and its transaction's signer keys.  A Leaf's child range is not read.
//
// TWO PATHS, the same result: a transaction whose max(nodes, 1) x max(signers, 1) is below wide_min is decided by ONE
// lane (cvck_narrow_tx); the others are appended to a list through a device counter and decided by ONE WAVE each
// (cvck_wide_*: signer keys staged in tiles of CV_CK_TILE, lanes striding over the Leaf nodes, then over the
// requirements).  Per-node flags live in the workspace, one byte per node, written before they are read and only by
// the lane that owns the node in that phase: nothing relies on what the workspace held.  Both paths compare first
// words and then whole keys: the work is nodes x signers compares, not a hash lookup — the binding bounds the size
// of a transaction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef CV_HD
#define CV_HD __host__ __device__ __forceinline__
#endif

#define CV_CK_LEAF 0
#define CV_CK_NODE 1
// signer keys per LDS tile of the wide path: one key per lane and staging pass (two coalesced 16-byte loads a lane,
// 2 KB a wave), so a workgroup of one wave holds 2 KB of LDS and the LDS never limits residency; in the compare loop
// every lane reads the SAME tile key, which the LDS broadcasts without bank conflicts.  A larger tile would only
// spare barriers, of which a 300-signer transaction has ten.
#define CV_CK_TILE 64
// wide_min 0: a lane's serial compares reach a wave's worth of staging and barriers at about 64 nodes x 64 signers
#define CV_CK_WIDE_DEFAULT 4096u
// req_missing
#define CVCK_FULFILLED 0
#define CVCK_MISSING 1
#define CVCK_MALFORMED 2
// tx_status (include/cordaverify.h CV_VS_*)
#define CVCK_VS_OK 0
#define CVCK_VS_BAD_SIGNATURE 1
#define CVCK_VS_MISSING 2
#define CVCK_VS_MALFORMED 3
// bits a lane collects over its requirements and signatures
#define CVCK_M_MALFORMED 1u
#define CVCK_M_BADSIG 2u
#define CVCK_M_NEEDED 4u
// workspace: the list's counter (16 bytes), the list (one word per transaction), the flags (one byte per node)
#define CVCK_WS_LIST 16

struct CvCk {
    uint32_t ntx, nreq, nnodes, nchild, nsig;
    const uint8_t *kind, *leaf_key;        // nnodes, nnodes * 32
    const int32_t *threshold;              // nnodes
    const uint32_t *child_begin, *child;   // nnodes + 1, nchild
    const int32_t *weight;                 // nchild
    const uint32_t *req_begin, *tx_req_begin;
    const uint8_t *sig_key;                // nsig * 32
    const uint32_t *tx_sig_begin;
    const uint8_t *req_allowed;            // nreq, or null = none
    const uint64_t *bitmap;                // verdict bits of the signatures, or null = all valid
    uint32_t wide_min;                     // resolved: never 0
    uint32_t *count, *list;                // workspace: transactions left to the wide path
    uint8_t *flag;                         // workspace: nnodes
    uint8_t *req_missing, *tx_status;
};

CV_HD uint64_t cvck_up16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }
CV_HD uint64_t cvck_ws_flag_off(uint64_t ntx) { return CVCK_WS_LIST + cvck_up16(4 * ntx); }
CV_HD uint64_t cvck_ws_bytes(uint64_t ntx, uint64_t nnodes) { return cvck_ws_flag_off(ntx) + cvck_up16(nnodes); }

// The first word of a 32-byte key, and the whole-key compare (two 16-byte loads a side on the device, where the
// records are 16-byte aligned; the host harness's arrays need no alignment).
CV_HD uint32_t cvck_word0(const uint8_t *k) {
#ifdef __HIP_DEVICE_COMPILE__
    return *reinterpret_cast<const uint32_t *>(k);
#else
    uint32_t w;
    __builtin_memcpy(&w, k, 4);
    return w;
#endif
}
CV_HD bool cvck_key_eq(const uint8_t *a, const uint8_t *b) {
#ifdef __HIP_DEVICE_COMPILE__
    const uint4 a0 = reinterpret_cast<const uint4 *>(a)[0], a1 = reinterpret_cast<const uint4 *>(a)[1];
    const uint4 b0 = reinterpret_cast<const uint4 *>(b)[0], b1 = reinterpret_cast<const uint4 *>(b)[1];
    return ((a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) | (a1.z ^ b1.z) |
            (a1.w ^ b1.w)) == 0;
#else
    return __builtin_memcmp(a, b, 32) == 0;
#endif
}

// Is `key` among n keys at `keys` (32 bytes each)?  First words first, the whole key only where they agree.
CV_HD bool cvck_key_among(const uint8_t *key, const uint8_t *keys, uint32_t n) {
    const uint32_t w = cvck_word0(key);
    for (uint32_t s = 0; s < n; s++)
        if (cvck_word0(keys + 32 * (size_t)s) == w && cvck_key_eq(key, keys + 32 * (size_t)s)) return true;
    return false;
}

// Node k of the requirement that starts at node rb, its children's flags written: CompositeKey.Node.isFulfilledBy.
// Returns its flag; *malformed is set (and the flag 0) when its child range or a child is out of bounds.
CV_HD uint8_t cvck_node(const CvCk &C, uint32_t rb, uint32_t k, bool *malformed) {
    const uint32_t cb = C.child_begin[k], ce = C.child_begin[k + 1];
    if (cb > ce || ce > C.nchild) {
        *malformed = true;
        return 0;
    }
    uint32_t sum = 0;                      // Kotlin's Int sum, wrapping
    for (uint32_t j = cb; j < ce; j++) {
        const uint32_t c = C.child[j];
        if (c < rb || c >= k) {
            *malformed = true;
            return 0;
        }
        if (C.flag[c]) sum += (uint32_t)C.weight[j];
    }
    return (int32_t)sum >= C.threshold[k] ? 1 : 0;
}

// Requirement r with its nodes in index order; LEAVES_DONE: the Leaf flags are already in C.flag (the wide path),
// else each Leaf is compared with the ns signer keys at `sigs` here.  Returns req_missing[r].
template <bool LEAVES_DONE>
CV_HD uint8_t cvck_requirement(const CvCk &C, uint32_t r, const uint8_t *sigs, uint32_t ns) {
    const uint32_t rb = C.req_begin[r], re = C.req_begin[r + 1];
    if (rb >= re) return CVCK_MALFORMED;
    bool bad = false;
    for (uint32_t k = rb; k < re; k++) {
        const uint8_t kd = C.kind[k];
        if (kd == CV_CK_LEAF) {
            if (!LEAVES_DONE) C.flag[k] = cvck_key_among(C.leaf_key + 32 * (size_t)k, sigs, ns) ? 1 : 0;
        } else if (kd == CV_CK_NODE) {
            C.flag[k] = cvck_node(C, rb, k, &bad);
        } else {
            bad = true;
            C.flag[k] = 0;
        }
    }
    if (bad) return CVCK_MALFORMED;
    return C.flag[re - 1] ? CVCK_FULFILLED : CVCK_MISSING;
}

// What requirement r adds to its transaction's bits, req_missing[r] given
CV_HD uint32_t cvck_req_bits(const CvCk &C, uint32_t r, uint8_t missing) {
    if (missing == CVCK_MALFORMED) return CVCK_M_MALFORMED;
    if (missing == CVCK_MISSING && !(C.req_allowed && C.req_allowed[r])) return CVCK_M_NEEDED;
    return 0;
}

// verdict bit of signature s (all valid without a bitmap)
CV_HD bool cvck_sig_valid(const CvCk &C, uint32_t s) { return !C.bitmap || ((C.bitmap[s >> 6] >> (s & 63u)) & 1u); }

// tx_status from the bits, first match wins: malformed, bad signature (none at all, or a 0 bit: the rule of
// cv_tx_verdicts, and checkSignaturesAreValid runs before the missing check), missing and not allowed, ok
CV_HD uint8_t cvck_status(uint32_t bits, uint32_t ns) {
    if (bits & CVCK_M_MALFORMED) return CVCK_VS_MALFORMED;
    if (ns == 0 || (bits & CVCK_M_BADSIG)) return CVCK_VS_BAD_SIGNATURE;
    if (bits & CVCK_M_NEEDED) return CVCK_VS_MISSING;
    return CVCK_VS_OK;
}

// max(nodes, 1) x max(signers, 1) of transaction t against wide_min (UINT32_MAX: never)
CV_HD bool cvck_is_wide(const CvCk &C, uint32_t t) {
    if (C.wide_min == 0xffffffffu) return false;
    const uint32_t nb = C.req_begin[C.tx_req_begin[t]], ne = C.req_begin[C.tx_req_begin[t + 1]];
    const uint32_t ns = C.tx_sig_begin[t + 1] - C.tx_sig_begin[t];
    const uint64_t work = (uint64_t)(ne > nb ? ne - nb : 1u) * (ns ? ns : 1u);
    return work >= C.wide_min;
}

CV_HD uint32_t cvck_list_push(uint32_t *count) {
#ifdef __HIP_DEVICE_COMPILE__
    return atomicAdd(count, 1u);
#else
    return (*count)++;
#endif
}

// ---------------------------------------------------------------- narrow path: one lane per transaction
CV_HD void cvck_narrow_tx(const CvCk &C, uint32_t t) {
    if (cvck_is_wide(C, t)) {
        C.list[cvck_list_push(C.count)] = t;     // at most ntx entries: each transaction is pushed once
        return;
    }
    const uint32_t sb = C.tx_sig_begin[t], ns = C.tx_sig_begin[t + 1] - sb;
    const uint8_t *sigs = C.sig_key + 32 * (size_t)sb;
    uint32_t bits = 0;
    for (uint32_t r = C.tx_req_begin[t]; r < C.tx_req_begin[t + 1]; r++) {
        const uint8_t m = cvck_requirement<false>(C, r, sigs, ns);
        C.req_missing[r] = m;
        bits |= cvck_req_bits(C, r, m);
    }
    for (uint32_t s = 0; s < ns; s++)
        if (!cvck_sig_valid(C, sb + s)) bits |= CVCK_M_BADSIG;
    C.tx_status[t] = cvck_status(bits, ns);
}

// ---------------------------------------------------------------- wide path: one wave per listed transaction
// The phases of transaction t, each run by all 64 lanes with a barrier between two of them:
//   clear            the Leaf flags of the lane's nodes (lanes stride over the transaction's nodes)
//   per tile i:      stage — lane j copies signer key i * CV_CK_TILE + j into the tile;
//                    match — the lane ORs into the flags of its Leaf nodes whether the key is in the tile
//   reqs             lanes stride over the requirements (Nodes in index order from the flags) and over the
//                    signatures' verdict bits; returns the lane's bits, ORed over the wave into tx_status
CV_HD void cvck_wide_clear(const CvCk &C, uint32_t t, uint32_t lane) {
    const uint32_t nb = C.req_begin[C.tx_req_begin[t]], ne = C.req_begin[C.tx_req_begin[t + 1]];
    for (uint32_t k = nb + lane; k < ne; k += 64)
        if (C.kind[k] == CV_CK_LEAF) C.flag[k] = 0;
}
// keys of tile i
CV_HD uint32_t cvck_tile_keys(const CvCk &C, uint32_t t, uint32_t i) {
    const uint32_t ns = C.tx_sig_begin[t + 1] - C.tx_sig_begin[t], done = i * CV_CK_TILE;
    return ns - done < CV_CK_TILE ? ns - done : CV_CK_TILE;
}
CV_HD uint32_t cvck_tiles(const CvCk &C, uint32_t t) {
    const uint32_t ns = C.tx_sig_begin[t + 1] - C.tx_sig_begin[t];
    return ns / CV_CK_TILE + (ns % CV_CK_TILE ? 1u : 0u);
}
CV_HD void cvck_wide_stage(const CvCk &C, uint32_t t, uint32_t i, uint32_t lane, uint8_t *tile) {
    if (lane >= cvck_tile_keys(C, t, i)) return;
    const uint8_t *src = C.sig_key + 32 * ((size_t)C.tx_sig_begin[t] + (size_t)i * CV_CK_TILE + lane);
#ifdef __HIP_DEVICE_COMPILE__
    reinterpret_cast<uint4 *>(tile + 32 * lane)[0] = reinterpret_cast<const uint4 *>(src)[0];
    reinterpret_cast<uint4 *>(tile + 32 * lane)[1] = reinterpret_cast<const uint4 *>(src)[1];
#else
    __builtin_memcpy(tile + 32 * lane, src, 32);
#endif
}
CV_HD void cvck_wide_match(const CvCk &C, uint32_t t, uint32_t i, uint32_t lane, const uint8_t *tile) {
    const uint32_t nb = C.req_begin[C.tx_req_begin[t]], ne = C.req_begin[C.tx_req_begin[t + 1]];
    const uint32_t nk = cvck_tile_keys(C, t, i);
    for (uint32_t k = nb + lane; k < ne; k += 64)
        if (C.kind[k] == CV_CK_LEAF && !C.flag[k] && cvck_key_among(C.leaf_key + 32 * (size_t)k, tile, nk)) C.flag[k] = 1;
}
CV_HD uint32_t cvck_wide_reqs(const CvCk &C, uint32_t t, uint32_t lane) {
    uint32_t bits = 0;
    for (uint32_t r = C.tx_req_begin[t] + lane; r < C.tx_req_begin[t + 1]; r += 64) {
        const uint8_t m = cvck_requirement<true>(C, r, nullptr, 0);
        C.req_missing[r] = m;
        bits |= cvck_req_bits(C, r, m);
    }
    for (uint32_t s = C.tx_sig_begin[t] + lane; s < C.tx_sig_begin[t + 1]; s += 64)
        if (!cvck_sig_valid(C, s)) bits |= CVCK_M_BADSIG;
    return bits;
}
