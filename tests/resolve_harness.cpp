// resolve_harness.cpp — TEST INFRASTRUCTURE: the graph half of cv_resolve_batch (corda_amd/csrc/cv_resolve.h: the
// per-lane core is __host__ __device__, the order and the walk are host code) on the CPU, for
// tests/test_resolve_cpu.py, which builds this file into tests/_build/libcvresolve.so, and for tests/resolve_san.cpp,
// which includes it.
//
// hrs_run runs the steps the launchers of cv_kernels.hip enqueue (cvk_resolve_join: insert, probe; cvk_resolve_gate)
// over a table and counters it prepares as cv_api_resolve.cpp does, each step's lanes ONE AFTER ANOTHER in the order
// `order` names — 0 ascending, 1 descending, 2 one fixed shuffle, 3 + k ascending from lane k on (so any lane can be
// made the first to claim a slot) — and then cvr_finish, the library's own host code.  The results must not depend on
// the order.  slots: 0 = the library's size (cvr_slots), else a power of two above ntx (an outside input's probe ends
// at an empty slot), to force collisions.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../corda_amd/csrc/cv_resolve.h"

namespace {

std::vector<uint32_t> lanes(size_t n, int order) {
    std::vector<uint32_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (uint32_t)(order == 1 ? n - 1 - i : order >= 3 ? (i + (size_t)(order - 3)) % n : i);
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

uint32_t hrs_slots(uint32_t ntx) { return cvr_slots(ntx); }

// 0, or -2 when a probe loop ran out of slots (the library's CV_E_HIP); -3 for a slot count that cannot hold the batch
int hrs_run(uint32_t ntx, uint32_t ninputs, const uint32_t *claimed, const uint32_t *tx_input_begin,
            const uint32_t *input_txhash, const uint32_t *input_index, const uint32_t *tx_output_count,
            const uint8_t *mstatus, const uint32_t *id, const uint32_t *tx_sig_begin, const uint64_t *bitmap,
            const uint8_t *sig_status, const uint8_t *sig_pre, const uint8_t *ck_status, uint64_t seed, uint32_t slots,
            int order, uint8_t *outcome, uint32_t *first_bad, uint32_t *bad_input, uint32_t *input_dep,
            uint8_t *input_status, uint32_t *order_out, uint32_t *graph) {
    if (slots == 0) slots = cvr_slots(ntx);
    if ((slots & (slots - 1)) || slots <= ntx) return -3;
    std::vector<uint32_t> tab(slots, CVR_NONE);
    uint32_t dstat[CVR_D_WORDS];
    for (int k = 0; k < CVR_D_WORDS; k++) dstat[k] = k < CVR_D_ERROR ? CVR_NONE : 0;
    CvResolve R{};
    R.ntx = ntx, R.ninputs = ninputs;
    R.claimed = claimed, R.tab = tab.data(), R.mask = slots - 1, R.seed = seed;
    R.tx_input_begin = tx_input_begin, R.input_txhash = input_txhash, R.input_index = input_index;
    R.tx_output_count = tx_output_count, R.input_dep = input_dep, R.input_status = input_status;
    R.mstatus = mstatus, R.id = id, R.tx_sig_begin = tx_sig_begin, R.bitmap = bitmap, R.sig_status = sig_status;
    R.sig_pre = sig_pre, R.ck_status = ck_status;
    R.outcome = outcome, R.first_bad = first_bad, R.bad_input = bad_input, R.dstat = dstat;
    for (uint32_t t : lanes(ntx, order)) cvr_insert(R, t);
    for (uint32_t i : lanes(ninputs, order)) cvr_probe(R, i);
    for (uint32_t t : lanes(ntx, order)) cvr_gate(R, t);
    return cvr_finish(ntx, tx_input_begin, input_dep, input_status, outcome, bad_input, dstat, order_out, graph) ? 0 : -2;
}

}  // extern "C"
