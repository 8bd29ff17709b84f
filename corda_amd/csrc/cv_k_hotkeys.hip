// cv_k_hotkeys.hip — the hot-key route's own steps (cv_hotkeys.h), one kernel per step, a lane per key or per record:
// tally, classify, keys, flag, gather, merge.  The compactions between them are the dedupe's count and scan kernels
// (cv_k_dedupe.hip).  Shared helpers and every kernel declaration: cv_kcommon.h; launchers: cv_kernels.hip
// (cvk_hotkeys_*).  No kernel here waits for another lane's store; the kernel boundaries publish each step's arrays.
#include "cv_kcommon.h"

// Before the counters: per wave, the lanes that carry one key_index elect their lowest lane, and that lane adds their
// number in one atomic — a batch of two keys would otherwise queue every record's atomic on two addresses (what
// DESIGN.md §5.14 measured at 0.6-0.95 ms in the dedupe's first form).  cv_dedupe_insert_kernel's rounds on one word
// instead of eight: the lowest lane still unmatched leads, its key_index goes round by a cross-lane read, the lanes
// that hold the same one are settled.  The rounds end after CVH_ELECT_ROUNDS, or as soon as a leader matches nobody
// but itself (a wave of distinct keys pays for one round); the lanes still unmatched then add for themselves.
#define CVH_ELECT_ROUNDS 4
__global__ __launch_bounds__(CV_BLOCK) void cv_hot_tally_kernel(CvHot H) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x, lane = threadIdx.x & 63u;
    bool open = i < H.n;
    const uint32_t k = open ? H.key_index[i] : 0u;
    for (int round = 0; round < CVH_ELECT_ROUNDS; round++) {
        const unsigned long long rest = __ballot(open);           // uniform over the wave, as is all that steers the loop
        if (!rest) break;
        const int leader = __ffsll(rest) - 1;
        const bool same = open && k == (uint32_t)__shfl((int)k, leader, 64);
        const uint32_t group = (uint32_t)__popcll(__ballot(same));
        if (same) {
            open = false;
            if (lane == (uint32_t)leader) cvh_tally(H, k, group);
        }
        if (group == 1) break;
    }
    if (open) cvh_tally(H, k, 1);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_hot_classify_kernel(CvHot H) {
    const uint32_t k = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (k < H.n) cvh_classify(H, k);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_hot_keys_kernel(CvHot H) {
    const uint32_t k = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (k < H.n) cvh_keys(H, k);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_hot_flag_kernel(CvHot H) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < H.n) cvh_flag(H, i);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_hot_gather_kernel(CvHot H) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < H.n) cvh_gather(H, i);
}

// A wave per 64-bit word of the caller's bitmap: the lanes past n contribute 0 (the zero tail bits), lane 0 stores the
// word whole, and a wave that starts at or past n stores nothing — exactly ceil(n / 64) words are written.
__global__ __launch_bounds__(CV_BLOCK) void cv_hot_merge_kernel(CvHot H, uint64_t *bitmap, uint8_t *status) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    const bool bit = i < H.n && cvh_merge(H, i, status) != 0;
    const unsigned long long word = __ballot(bit);
    if ((threadIdx.x & 63u) == 0 && i < H.n) bitmap[i >> 6] = word;
}
