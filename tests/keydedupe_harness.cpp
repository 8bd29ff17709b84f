// keydedupe_harness.cpp — TEST INFRASTRUCTURE: the device key dedupe (corda_amd/csrc/cv_keydedupe.h: the per-lane core
// is __host__ __device__) on the CPU, for tests/test_keydedupe_cpu.py, which builds this file into
// tests/_build/libcvkeydedupe.so, and for tests/keydedupe_san.cpp, which includes it.
//
// hkd_run runs the steps the launcher of cv_kernels.hip enqueues (cvk_dedupe: the table and stat cleared to 0xff,
// insert, mark, the compaction of the flags, emit) over a workspace laid out as the library lays it out, each step's
// lanes ONE AFTER ANOTHER in the order `order` names — 0 ascending, 1 descending, 2 one fixed shuffle.  The results
// must not depend on the order, the seed or the table's size.  The compaction's count and scan kernels are block-wide
// device code (cv_k_dedupe.hip; tests/test_gpu_keydedupe.py runs them at every level); here the flags' exclusive
// prefix sums are taken block by block of CVD_SPAN entries from the blocks' scanned sums, the same recursion.
// slots: 0 = the library's size (cvd_slots), else a power of two of at least n, to force collisions up to a full table.
// *wrapped: 1 when some key lies in a slot below its home slot, so its probe passed the table's last slot.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../corda_amd/csrc/cv_keydedupe.h"

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

// cvk_dedupe's dedupe_scan: arr -> its exclusive prefix sums in place, *total = the sum
void scan_levels(std::vector<uint32_t> &arr, uint32_t *total) {
    const size_t m = arr.size();
    if (m <= CVD_SPAN) {
        uint32_t run = 0;
        for (size_t i = 0; i < m; i++) {
            const uint32_t v = arr[i];
            arr[i] = run;
            run += v;
        }
        *total = run;
        return;
    }
    std::vector<uint32_t> sums(cvd_blocks(m), 0);
    for (size_t i = 0; i < m; i++) sums[i / CVD_SPAN] += arr[i];
    scan_levels(sums, total);
    for (size_t b = 0; b < sums.size(); b++) {
        uint32_t run = sums[b];
        for (size_t i = b * CVD_SPAN; i < m && i < (b + 1) * CVD_SPAN; i++) {
            const uint32_t v = arr[i];
            arr[i] = run;
            run += v;
        }
    }
}

}  // namespace

extern "C" {

uint64_t hkd_slots(uint64_t n) { return cvd_slots(n); }
uint64_t hkd_workspace(uint64_t n) { return cvd_layout(n).bytes; }

// 0, or -2 after a probe error (nkeys = CVD_NONE: the library's CV_E_HIP); -3 for a slot count that cannot hold the batch
int hkd_run(uint32_t n, const uint32_t *pk, uint64_t seed, uint64_t slots, int order, uint32_t *keys, uint32_t *key_index,
            uint32_t *nkeys, int *wrapped) {
    if (n == 0) return -3;
    CvdLayout L = cvd_layout(n);
    if (slots) {
        if ((slots & (slots - 1)) || slots < n) return -3;
        L.slots = slots;
    }
    // table | stat in one block, as the one memset of the launcher needs them; the other pieces sized exactly
    std::vector<uint32_t> tab(L.slots + CVD_STAT_WORDS, CVD_NONE), first(n, 0xEEEEEEEEu), number(n, 0xEEEEEEEEu);
    CvDedupe D{};
    D.n = n, D.pk = pk, D.tab = tab.data(), D.mask = L.slots - 1, D.seed = seed, D.stat = tab.data() + L.slots;
    D.first = first.data(), D.number = number.data(), D.keys = keys, D.key_index = key_index, D.nkeys = nkeys;
    for (uint32_t i : lanes(n, order)) cvd_insert(D, i);
    for (uint32_t i : lanes(n, order)) cvd_mark(D, i);
    scan_levels(number, D.stat + CVD_STAT_TOTAL);
    for (uint32_t i : lanes(n, order)) cvd_emit(D, i);
    if (wrapped) {
        *wrapped = 0;
        for (uint64_t s = 0; s < L.slots; s++)
            if (tab[s] != CVD_NONE && (cvu_hash(pk + 8 * (size_t)tab[s], seed) & D.mask) > s) *wrapped = 1;
    }
    return *nkeys == CVD_NONE ? -2 : 0;
}

}  // extern "C"
