// notary_harness.cpp — TEST INFRASTRUCTURE: the per-lane decisions of cv_notarise_batch (corda_amd/csrc/cv_notary.h;
// __host__ __device__) on the CPU, for tests/test_notary_cpu.py, which builds this file into
// tests/_build/libcvnotary.so, and for tests/notary_san.cpp, which includes it.
//
// hnt_gate / hnt_gather / hnt_final run the steps the launchers of cv_kernels.hip enqueue (cvk_notary_gate, _gather,
// _final), each step's lanes ONE AFTER ANOTHER in the order `order` names: 0 ascending, 1 descending, 2 one fixed
// shuffle.  The results must not depend on it.  The finalise kernel's block scan is a running count here: a lane's
// place in the list is the number of accepted transactions before it.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../corda_amd/csrc/cv_notary.h"

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

// tx_pre, sig_pre may be null; the signature arrays are read only when validating
void hnt_gate(uint32_t ntx, int validating, const uint8_t *mstatus, const uint32_t *id, const uint32_t *claimed,
              const uint8_t *tx_pre, const uint32_t *tx_sig_begin, const uint64_t *bitmap, const uint8_t *sig_status,
              const uint8_t *sig_pre, const uint8_t *ck_status, int order, uint8_t *pre, uint8_t *enable,
              uint32_t *first_bad) {
    CvNotary N{};
    N.ntx = ntx, N.validating = validating;
    N.mstatus = mstatus, N.id = id, N.claimed = claimed, N.tx_pre = tx_pre;
    N.tx_sig_begin = tx_sig_begin, N.bitmap = bitmap, N.sig_status = sig_status, N.sig_pre = sig_pre;
    N.ck_status = ck_status;
    N.pre = pre, N.enable = enable, N.first_bad = first_bad;
    for (uint32_t t : lanes(ntx, order)) cvn_gate(N, t);
}

void hnt_gather(uint32_t nstates, const uint32_t *leaf_digest, const uint32_t *state_leaf, int order, uint32_t *key) {
    CvNotary N{};
    N.nstates = nstates;
    N.leaf_digest = leaf_digest, N.state_leaf = state_leaf, N.key = key;
    for (uint32_t i : lanes(nstates, order)) cvn_gather(N, i);
}

// returns the number of accepted transactions; list, sign_off and sign_len get that many entries
uint32_t hnt_final(uint32_t ntx, const uint8_t *pre, const uint8_t *uniq_status, int order, uint8_t *outcome,
                   uint32_t *list, uint64_t *sign_off, uint32_t *sign_len) {
    CvNotary N{};
    N.ntx = ntx;
    N.pre = const_cast<uint8_t *>(pre), N.uniq_status = uniq_status, N.outcome = outcome;
    N.list = list, N.sign_off = sign_off, N.sign_len = sign_len;
    std::vector<uint32_t> acc(ntx), pos(ntx);
    for (uint32_t t : lanes(ntx, order)) acc[t] = cvn_final(N, t);
    uint32_t count = 0;
    for (uint32_t t = 0; t < ntx; t++) {
        pos[t] = count;
        count += acc[t];
    }
    for (uint32_t t : lanes(ntx, order))
        if (acc[t]) cvn_place(N, t, pos[t]);
    return count;
}

}  // extern "C"
