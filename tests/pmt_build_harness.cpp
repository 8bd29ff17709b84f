// pmt_build_harness.cpp — TEST INFRASTRUCTURE: the partial Merkle tree build core of corda_amd/csrc/cv_pmt_build.h
// (cv_pmtb_count, cv_pmtb_emit; __host__ __device__) on the CPU, for tests/test_pmt_build.py, which builds this file
// into tests/_build/libcvpmtb.so, and for tests/pmt_build_san.cpp, which includes it.
//
// cvb_build does for a batch what the three kernels of cv_k_pmt.hip do: per transaction the count sweep over its
// level pyramid, then the exclusive sum of the node counts, then the emit sweep — the same procedures, one
// transaction after another.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../corda_amd/csrc/cv_pmt_build.h"

extern "C" {

uint64_t cvb_bound(uint32_t L) { return cv_pmtb_bound(L); }
uint64_t cvb_pyramid(uint32_t L) { return cv_pmtb_pyramid_entries(L); }

// leaf_hash[nleaves][32] cut by txb[ntx + 1]; include[.][32] cut by inc_begin[ntx + 1], or keep[nleaves] when keep is
// non-null.  The node arrays must hold the batch's bound.  Returns the number of nodes written.
uint32_t cvb_build(uint32_t ntx, const uint8_t *leaf_hash, const uint32_t *txb, const uint8_t *include,
                   const uint32_t *inc_begin, const uint8_t *keep, uint8_t *kind, uint32_t *left, uint32_t *right,
                   uint8_t *node_hash, uint32_t *tree_begin, uint8_t *ids, uint8_t *status) {
    std::vector<size_t> ws_off(ntx + 1, 0);
    for (uint32_t t = 0; t < ntx; t++) ws_off[t + 1] = ws_off[t] + (size_t)cv_pmtb_pyramid_entries(txb[t + 1] - txb[t]);
    const size_t P = ws_off[ntx];
    std::vector<uint32_t> dig(8 * P + 8), size(P + 1), pos(P + 1), count(ntx + 1);
    std::vector<uint8_t> flag(P + 1);
    for (uint32_t t = 0; t < ntx; t++) {
        const uint32_t lb = txb[t], L = txb[t + 1] - lb;
        const size_t w = ws_off[t];
        for (uint32_t i = 0; i < L; i++) cv_load_digest(&dig[8 * (w + i)], leaf_hash + 32 * (size_t)(lb + i));
        uint32_t root[8];
        const uint32_t ib = keep ? 0 : inc_begin[t], ie = keep ? 0 : inc_begin[t + 1];
        status[t] = (uint8_t)cv_pmtb_count(L, &dig[8 * w], &flag[w], &size[w], &pos[w],
                                           keep ? nullptr : include + 32 * (size_t)ib, ie - ib,
                                           keep ? keep + lb : nullptr, root, count[t]);
        for (int q = 0; q < 8; q++) {
            const uint32_t be = cv_bswap32(root[q]);
            memcpy(ids + 32 * (size_t)t + 4 * q, &be, 4);
        }
    }
    uint32_t sum = 0;
    for (uint32_t t = 0; t < ntx; t++) {
        tree_begin[t] = sum;
        sum += count[t];
    }
    tree_begin[ntx] = sum;
    for (uint32_t t = 0; t < ntx; t++) {
        if (status[t] != CV_PMTB_OK) continue;
        const size_t w = ws_off[t];
        cv_pmtb_emit(txb[t + 1] - txb[t], &dig[8 * w], &flag[w], &size[w], &pos[w], tree_begin[t], kind, left, right,
                     node_hash);
    }
    return sum;
}

// cv_pmt_verify (cv_verify.h) of nodes [b, e) against root and check[cb .. ce): verdict | status << 8
int cvb_verify(uint32_t b, uint32_t e, const uint8_t *kind, const uint32_t *left, const uint32_t *right,
               const uint8_t *node_hash, const uint8_t *root, const uint8_t *check, uint32_t cb, uint32_t ce) {
    std::vector<uint32_t> dig(8 * (size_t)e + 8);
    std::vector<uint8_t> flag((size_t)e + 1);
    bool v = false;
    const int st = cv_pmt_verify(b, e, kind, left, right, node_hash, root, check, cb, ce, dig.data(), flag.data(), v);
    return (v ? 1 : 0) | (st << 8);
}

// the Merkle root of L leaf hashes by cv_merkle_root_inplace (the id kernel's procedure); false for no leaves
int cvb_root(uint32_t L, const uint8_t *leaf_hash, uint8_t *root) {
    std::vector<uint32_t> lvl(8 * (size_t)L + 8);
    for (uint32_t i = 0; i < L; i++) cv_load_digest(&lvl[8 * (size_t)i], leaf_hash + 32 * (size_t)i);
    uint32_t r[8];
    const bool ok = cv_merkle_root_inplace(lvl.data(), L, r);
    for (int q = 0; q < 8; q++) {
        const uint32_t be = cv_bswap32(r[q]);
        memcpy(root + 4 * q, &be, 4);
    }
    return ok ? 1 : 0;
}

}  // extern "C"
