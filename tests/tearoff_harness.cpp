// tearoff_harness.cpp — TEST INFRASTRUCTURE: the per-lane decisions of cv_filtered_verify and cv_tearoff_sign_batch
// (corda_amd/csrc/cv_tearoff.h; __host__ __device__) on the CPU, for tests/test_tearoff_cpu.py, which builds this file
// into tests/_build/libcvtearoff.so, and for tests/tearoff_san.cpp, which includes it.
//
// htf_check / htf_gate / htf_compact run the steps the launchers of cv_kernels.hip enqueue (cvk_tearoff_check, _gate,
// _compact), each step's lanes ONE AFTER ANOTHER in the order `order` names: 0 ascending, 1 descending, 2 one fixed
// shuffle.  The results must not depend on it.  The compaction kernel's block scan is a running count here: a lane's
// place in the list is the number of accepted tear-offs before it.  htf_leaf_digests and htf_verify stand in for the
// two existing kernels between them (the leaf kernel's SHA-256, cv_sha.h, and cv_pmt_verify, cv_verify.h), so a test
// can run the whole chain from the leaf blobs on.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../corda_amd/csrc/cv_verify.h"
#include "../corda_amd/csrc/cv_tearoff.h"

namespace {

std::vector<uint32_t> lanes(size_t n, int order) {
    std::vector<uint32_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (uint32_t)(order == 1 ? n - 1 - i : i);
    if (order == 2) {
        uint64_t x = 0x9e3779b97f4a7c15ull;
        for (size_t i = n; i > 1; i--) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(v[i - 1], v[(size_t)((x >> 33) % i)]);
        }
    }
    return v;
}

}  // namespace

extern "C" {

// the digests as the leaf kernel leaves them: 8 big-endian state words a leaf
void htf_leaf_digests(uint32_t nleaves, const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint32_t *digest) {
    for (uint32_t i = 0; i < nleaves; i++) sha256_bytes(digest + 8 * (size_t)i, arena + off[i], len[i]);
}

void htf_check(uint32_t nleaves, const uint32_t *leaf_digest, int order, uint32_t *check) {
    CvTearoff T{};
    T.nleaves = nleaves;
    T.leaf_digest = leaf_digest, T.check = check;
    for (uint32_t i : lanes(nleaves, order)) cvt_check(T, i);
}

// cv_pmt_verify_kernel's lane for every tree
void htf_verify(uint32_t ntx, uint32_t nnodes, const uint8_t *kind, const uint32_t *left, const uint32_t *right,
                const uint8_t *node_hash, const uint32_t *tree_begin, const uint8_t *root, const uint8_t *check,
                const uint32_t *check_begin, uint8_t *verdict, uint8_t *status) {
    std::vector<uint32_t> dig(8 * (size_t)nnodes + 8);
    std::vector<uint8_t> flag((size_t)nnodes + 1);
    for (uint32_t t = 0; t < ntx; t++) {
        bool v = false;
        status[t] = (uint8_t)cv_pmt_verify(tree_begin[t], tree_begin[t + 1], kind, left, right, node_hash,
                                           root + 32 * (size_t)t, check, check_begin[t], check_begin[t + 1], dig.data(),
                                           flag.data(), v);
        verdict[t] = v ? 1 : 0;
    }
}

// leaf_pre, fv_verdict and fv_status may be null
void htf_gate(uint32_t ntx, const uint32_t *tx_leaf_begin, const uint8_t *verdict, const uint8_t *status,
              const uint8_t *leaf_pre, int order, uint8_t *fv_verdict, uint8_t *fv_status, uint8_t *outcome,
              uint32_t *first_bad) {
    CvTearoff T{};
    T.ntx = ntx;
    T.tx_leaf_begin = tx_leaf_begin, T.verdict = verdict, T.status = status, T.leaf_pre = leaf_pre;
    T.fv_verdict = fv_verdict, T.fv_status = fv_status, T.outcome = outcome, T.first_bad = first_bad;
    for (uint32_t t : lanes(ntx, order)) cvt_gate(T, t);
}

// returns the number of accepted tear-offs; list, sign_off and sign_len get that many entries
uint32_t htf_compact(uint32_t ntx, const uint8_t *outcome, int order, uint32_t *list, uint64_t *sign_off,
                     uint32_t *sign_len) {
    CvTearoff T{};
    T.ntx = ntx;
    T.outcome = const_cast<uint8_t *>(outcome);
    T.list = list, T.sign_off = sign_off, T.sign_len = sign_len;
    std::vector<uint32_t> acc(ntx), pos(ntx);
    for (uint32_t t : lanes(ntx, order)) acc[t] = cvt_accepted(T, t);
    uint32_t count = 0;
    for (uint32_t t = 0; t < ntx; t++) {
        pos[t] = count;
        count += acc[t];
    }
    for (uint32_t t : lanes(ntx, order))
        if (acc[t]) cvt_place(T, t, pos[t]);
    return count;
}

}  // extern "C"
