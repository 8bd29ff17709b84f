// ck_harness.cpp — TEST INFRASTRUCTURE: the missing-signers per-lane core (corda_amd/csrc/cv_ck.h; __host__ __device__)
// on the CPU, for tests/test_ck_cpu.py, which builds this file into tests/_build/libcvck.so, and for tests/ck_san.cpp,
// which includes it.
//
// hck_run does what cvk_ck (cv_kernels.hip) enqueues: the list's counter cleared, the narrow kernel's lanes (one per
// transaction), then the wide kernel's waves (one per listed transaction, the phases of cv_k_ck.hip with the barriers
// where that has them), every phase's lanes ONE AFTER ANOTHER in the order `order` names: 0 ascending, 1 descending,
// 2 one fixed shuffle.  The results must not depend on it.  The workspace has exactly cvck_ws_bytes bytes and is
// filled with 0xA5 first: nothing may rely on its contents.  Returns the number of transactions the wide path decided.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../corda_amd/csrc/cv_ck.h"

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

uint64_t hck_workspace(uint64_t ntx, uint64_t nnodes) { return cvck_ws_bytes(ntx, nnodes); }
uint32_t hck_tile() { return CV_CK_TILE; }
uint32_t hck_wide_default() { return CV_CK_WIDE_DEFAULT; }

int64_t hck_run(uint32_t ntx, uint32_t nreq, uint32_t nnodes, uint32_t nchild, uint32_t nsig, const uint8_t *kind,
                const uint8_t *leaf_key, const int32_t *threshold, const uint32_t *child_begin, const uint32_t *child,
                const int32_t *weight, const uint32_t *req_begin, const uint32_t *tx_req_begin, const uint8_t *sig_key,
                const uint32_t *tx_sig_begin, const uint8_t *req_allowed, const uint64_t *bitmap, uint32_t wide_min,
                int order, uint8_t *req_missing, uint8_t *tx_status) {
    if (ntx == 0) return 0;
    // uint32_t storage: the counter and the list are words
    std::vector<uint32_t> ws((size_t)(cvck_ws_bytes(ntx, nnodes) / 4), 0xA5A5A5A5u);
    uint8_t *wsb = reinterpret_cast<uint8_t *>(ws.data());
    CvCk C{};
    C.ntx = ntx, C.nreq = nreq, C.nnodes = nnodes, C.nchild = nchild, C.nsig = nsig;
    C.kind = kind, C.leaf_key = leaf_key, C.threshold = threshold, C.child_begin = child_begin, C.child = child;
    C.weight = weight, C.req_begin = req_begin, C.tx_req_begin = tx_req_begin, C.sig_key = sig_key;
    C.tx_sig_begin = tx_sig_begin, C.req_allowed = req_allowed, C.bitmap = bitmap;
    C.wide_min = wide_min ? wide_min : CV_CK_WIDE_DEFAULT;
    C.count = ws.data(), C.list = ws.data() + CVCK_WS_LIST / 4, C.flag = wsb + cvck_ws_flag_off(ntx);
    C.req_missing = req_missing, C.tx_status = tx_status;
    *C.count = 0;                                                 // the launcher's hipMemsetAsync
    for (uint32_t t : lanes(ntx, order)) cvck_narrow_tx(C, t);
    if (C.wide_min == 0xffffffffu) return *C.count ? -1 : 0;      // the launcher skips the wide kernel
    const uint32_t listed = *C.count;
    if (listed > ntx) return -1;
    const std::vector<uint32_t> ln = lanes(64, order);
    std::vector<uint8_t> tile(CV_CK_TILE * 32);
    for (uint32_t i : lanes(listed, order)) {                     // the waves in any order too
        const uint32_t t = C.list[i];
        if (t >= ntx) return -1;
        std::fill(tile.begin(), tile.end(), 0x5A);
        for (uint32_t l : ln) cvck_wide_clear(C, t, l);
        const uint32_t tiles = cvck_tiles(C, t);
        for (uint32_t j = 0; j < tiles; j++) {
            for (uint32_t l : ln) cvck_wide_stage(C, t, j, l, tile.data());
            for (uint32_t l : ln) cvck_wide_match(C, t, j, l, tile.data());
        }
        uint32_t all = 0;
        for (uint32_t l : ln) all |= cvck_wide_reqs(C, t, l);
        tx_status[t] = cvck_status(all, tx_sig_begin[t + 1] - tx_sig_begin[t]);
    }
    return listed;
}

}  // extern "C"
