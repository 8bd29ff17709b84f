// cv_pmt_build.h — PartialMerkleTree.build over the full tree of MerkleTree.getMerkleTree, one transaction per
// lane (core/src/main/kotlin/net/corda/core/crypto/PartialMerkleTree.kt:69-111 over
// core/.../transactions/MerkleTransaction.kt:66-99; behind FilteredTransaction.buildMerkleTransaction,
// MerkleTransaction.kt:146-168).  The output is the flat post-order encoding cv_pmt_verify (cv_verify.h) reads.
//
// No recursion, no stack: three sweeps over the transaction's LEVEL PYRAMID, kept in workspace.  Level 0 is the
// L leaf digests, level l + 1 has ceil(n_l / 2) nodes, the last level is the root; node j of a level sits at
// pyramid index (level base) + j, the levels back to back (P(L) = sum of n_l entries).  Per entry: the digest
// (8 big-endian words), a flag byte (an included leaf lies below), the size of its subtree in the OUTPUT and its
// output position.
//   count : marks the leaves whose digest is in the include list, builds every level bottom-up with
//           flag = flag(left) | flag(right) and size = flag ? 1 + size(left) + size(right) : 1 — a level's odd last
//           node takes a DuplicatedLeaf as right sibling, which carries no flag and has size 1 — and sets the
//           status: the build fails iff the number of marked leaves differs from the include list's length
//   (scan : the exclusive sum of the transactions' node counts = where each tree begins, done by the caller)
//   emit  : top-down from pos(root) = begin + size - 1: a flagged node at p is a Node with right = p - 1 and
//           left = p - 1 - size(right), an unflagged one a Leaf with its hash, a DuplicatedLeaf a Leaf with its
//           left sibling's hash, a level-0 node an IncludedLeaf or a Leaf.  Entries no flagged parent leads to
//           keep pos = CV_PMTB_UNREACHED and write nothing.
// Every output record of [begin, begin + size(root)) is written exactly once, all of its fields.
#pragma once
#include "cv_verify.h"

#define CV_PMTB_OK 0
#define CV_PMTB_EMPTY 1          // no leaves: "Cannot calculate Merkle root on empty hash list."
#define CV_PMTB_NOT_IN_TREE 3    // "Some of the provided hashes are not in the tree."
#define CV_PMTB_UNREACHED 0xffffffffu

// nodes of level l of a tree over L leaves: l times ceil(n / 2) = ceil(L / 2^l)
CV_HD uint32_t cv_pmtb_level_count(uint32_t L, uint32_t l) {
    return (uint32_t)(((uint64_t)L + ((1ull << l) - 1)) >> l);
}

// P(L): entries of the level pyramid (0 for no leaves)
CV_HD uint64_t cv_pmtb_pyramid_entries(uint32_t L) {
    uint64_t p = 0;
    for (uint32_t n = L; n > 0; n = (n + 1) >> 1) {
        p += n;
        if (n == 1) break;
    }
    return p;
}

// the most nodes a build over L leaves emits: P(L) + D(L), D = the levels with an odd count above 1 (one
// DuplicatedLeaf each); reached when every leaf is included
CV_HD uint64_t cv_pmtb_bound(uint32_t L) {
    uint64_t p = 0;
    for (uint32_t n = L; n > 0; n = (n + 1) >> 1) {
        p += n;
        if (n == 1) break;
        p += n & 1u;
    }
    return p;
}

CV_HD bool cv_pmtb_digest_eq(const uint32_t *a, const uint32_t c[8]) {
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) diff |= a[q] ^ c[q];
    return diff == 0;
}

// Sweep 1 of one transaction.  dig / flag / size / pos: its pyramid (P(L) entries), level 0 of dig already holding
// the leaf digests.  The include list is either include[ninc][32] (keep == nullptr), or the transaction's own
// kept leaves: keep[L], non-zero = kept (include and ninc ignored), so a leaf is included iff its digest equals a
// kept leaf's and the list's length is the number of kept leaves.  root: the Merkle root (zero for no leaves);
// count: the nodes the emit sweep will write (0 unless the status is CV_PMTB_OK).  Returns the status.
__host__ __device__ inline int cv_pmtb_count(uint32_t L, uint32_t *dig, uint8_t *flag, uint32_t *size, uint32_t *pos,
                                             const uint8_t *include, uint32_t ninc, const uint8_t *keep,
                                             uint32_t root[8], uint32_t &count) {
    count = 0;
    if (L == 0) {
#pragma unroll
        for (int q = 0; q < 8; q++) root[q] = 0;
        return CV_PMTB_EMPTY;
    }
    for (uint32_t i = 0; i < L; i++) {
        flag[i] = 0;
        size[i] = 1;
        pos[i] = CV_PMTB_UNREACHED;
    }
    // membership by hash, not by position: every leaf equal to a listed hash is marked
    if (keep) {
        ninc = 0;
        for (uint32_t j = 0; j < L; j++) {
            if (!keep[j]) continue;
            ninc++;
            uint32_t c[8];
#pragma unroll
            for (int q = 0; q < 8; q++) c[q] = dig[8 * (size_t)j + q];
            for (uint32_t i = 0; i < L; i++)
                if (cv_pmtb_digest_eq(dig + 8 * (size_t)i, c)) flag[i] = 1;
        }
    } else {
        for (uint32_t j = 0; j < ninc; j++) {
            uint32_t c[8];
            cv_load_digest(c, include + 32 * (size_t)j);
            for (uint32_t i = 0; i < L; i++)
                if (cv_pmtb_digest_eq(dig + 8 * (size_t)i, c)) flag[i] = 1;
        }
    }
    uint32_t marked = 0;
    for (uint32_t i = 0; i < L; i++) marked += flag[i];
    // every level, kept: level base b, n nodes; the next level starts at b + n
    uint32_t b = 0, n = L;
    while (n > 1) {
        const uint32_t m = (n + 1) >> 1;
        for (uint32_t j = 0; j < m; j++) {
            const uint32_t li = b + 2 * j;
            const bool has_r = 2 * j + 1 < n;            // else a DuplicatedLeaf with the left node's hash
            const uint32_t ri = has_r ? li + 1 : li, k = b + n + j;
            uint32_t l[8], r[8], o[8];
#pragma unroll
            for (int q = 0; q < 8; q++) { l[q] = dig[8 * (size_t)li + q]; r[q] = dig[8 * (size_t)ri + q]; }
            sha256_node(o, l, r);
#pragma unroll
            for (int q = 0; q < 8; q++) dig[8 * (size_t)k + q] = o[q];
            const uint8_t f = (uint8_t)(flag[li] | (has_r ? flag[ri] : 0));
            flag[k] = f;
            size[k] = f ? 1 + size[li] + (has_r ? size[ri] : 1) : 1;
            pos[k] = CV_PMTB_UNREACHED;
        }
        b += n;
        n = m;
    }
#pragma unroll
    for (int q = 0; q < 8; q++) root[q] = dig[8 * (size_t)b + q];
    if (marked != ninc) return CV_PMTB_NOT_IN_TREE;
    count = size[b];
    return CV_PMTB_OK;
}

CV_HD void cv_pmtb_put(uint32_t p, uint8_t kd, uint32_t l, uint32_t r, const uint32_t *d, uint8_t *kind, uint32_t *left,
                       uint32_t *right, uint8_t *node_hash) {
    kind[p] = kd;
    left[p] = l;
    right[p] = r;
    uint32_t *h = reinterpret_cast<uint32_t *>(node_hash + 32 * (size_t)p);   // node_hash is 4-byte aligned
#pragma unroll
    for (int q = 0; q < 8; q++) h[q] = d ? cv_bswap32(d[q]) : 0u;
}

// Sweep 3 of one transaction whose status is CV_PMTB_OK (L >= 1): its tree into records
// [begin, begin + size(root)) of kind / left / right / node_hash (absolute indices, the root last).
__host__ __device__ inline void cv_pmtb_emit(uint32_t L, const uint32_t *dig, const uint8_t *flag, const uint32_t *size,
                                             uint32_t *pos, uint32_t begin, uint8_t *kind, uint32_t *left,
                                             uint32_t *right, uint8_t *node_hash) {
    uint32_t top = 0;
    while (cv_pmtb_level_count(L, top) > 1) top++;
    uint32_t b = (uint32_t)cv_pmtb_pyramid_entries(L) - 1;      // the root's entry = the top level's base
    pos[b] = begin + size[b] - 1;
    for (uint32_t lv = top; lv >= 1; lv--) {
        const uint32_t n = cv_pmtb_level_count(L, lv), nc = cv_pmtb_level_count(L, lv - 1), cb = b - nc;
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t k = b + j, p = pos[k];
            if (p == CV_PMTB_UNREACHED) continue;
            if (!flag[k]) {
                cv_pmtb_put(p, CV_PMT_LEAF, 0, 0, dig + 8 * (size_t)k, kind, left, right, node_hash);
                continue;
            }
            const uint32_t li = cb + 2 * j;
            const bool has_r = 2 * j + 1 < nc;
            const uint32_t rs = has_r ? size[li + 1] : 1;
            cv_pmtb_put(p, CV_PMT_NODE, p - 1 - rs, p - 1, nullptr, kind, left, right, node_hash);
            pos[li] = p - 1 - rs;
            if (has_r)
                pos[li + 1] = p - 1;
            else
                cv_pmtb_put(p - 1, CV_PMT_LEAF, 0, 0, dig + 8 * (size_t)li, kind, left, right, node_hash);
        }
        b = cb;
    }
    for (uint32_t i = 0; i < L; i++) {
        const uint32_t p = pos[i];
        if (p != CV_PMTB_UNREACHED)
            cv_pmtb_put(p, flag[i] ? CV_PMT_INCLUDED : CV_PMT_LEAF, 0, 0, dig + 8 * (size_t)i, kind, left, right, node_hash);
    }
}
