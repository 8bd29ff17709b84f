// cv_k_dedupe.hip — the device key dedupe (cv_keydedupe.h): one kernel per step — the table's insert, mark and emit (a
// lane per signature) and the ordered compaction's count and scan (a block per CVD_SPAN entries, CVD_PER consecutive
// entries per lane).  Shared helpers and every kernel declaration: cv_kcommon.h; launcher: cv_kernels.hip
// (cvk_dedupe).  No kernel here waits for another lane's store; the kernel boundaries publish the table, the flags
// and the block sums.
#include "cv_kcommon.h"

static_assert(CVD_SPAN == CV_BLOCK * CVD_PER, "a block of the compaction covers CVD_SPAN entries");

// Before the table: per wave, the lanes that carry one key elect their lowest lane — the smallest index among them —
// and only that lane inserts.  One round per key: the lowest lane still unmatched is the leader, its eight key words
// go round by cross-lane reads, the lanes that hold the same words are settled.  The rounds serve the batches of a
// handful of keys, whose lanes would otherwise queue on one slot's atomics; they end after CVD_ELECT_ROUNDS, or as
// soon as a leader matches nobody but itself (a wave of distinct keys pays for one round), and the lanes still
// unmatched then insert for themselves.  A lane that stands back always has a lower lane with its key that inserts.
#define CVD_ELECT_ROUNDS 4
__global__ __launch_bounds__(CV_BLOCK) void cv_dedupe_insert_kernel(CvDedupe D) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t k[8];
    bool open = i < D.n, leads = false;
#pragma unroll
    for (int q = 0; q < 8; q++) k[q] = open ? D.pk[8 * (size_t)i + q] : 0u;
    for (int round = 0; round < CVD_ELECT_ROUNDS; round++) {
        const unsigned long long rest = __ballot(open);           // uniform over the wave, as is all that steers the loop
        if (!rest) break;
        const int leader = __ffsll(rest) - 1;
        uint32_t diff = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) diff |= k[q] ^ __shfl(k[q], leader, 64);
        const bool same = open && diff == 0;
        if (same) {
            open = false;
            leads = lane == (uint32_t)leader;
        }
        if (__popcll(__ballot(same)) == 1) break;
    }
    if (leads || open) cvd_insert(D, i);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_dedupe_mark_kernel(CvDedupe D) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < D.n) cvd_mark(D, i);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_dedupe_emit_kernel(CvDedupe D) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < D.n) cvd_emit(D, i);
}

// the lane's CVD_PER entries of arr[0..m) (zero past the end) and their sum
__device__ __forceinline__ uint32_t cvd_load(uint32_t m, const uint32_t *__restrict__ arr, uint64_t i0, uint32_t v[CVD_PER]) {
    uint32_t own = 0;
#pragma unroll
    for (uint32_t q = 0; q < CVD_PER; q++) {
        v[q] = i0 + q < m ? arr[i0 + q] : 0u;
        own += v[q];
    }
    return own;
}

// sums[b] = the sum of block b's entries of arr[0..m): a wave reduction, the four wave sums through LDS
__global__ __launch_bounds__(CV_BLOCK) void cv_dedupe_count_kernel(uint32_t m, const uint32_t *__restrict__ arr,
                                                                   uint32_t *__restrict__ sums) {
    __shared__ uint32_t wsum[CV_BLOCK / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint32_t v[CVD_PER];
    uint32_t s = cvd_load(m, arr, (uint64_t)blockIdx.x * CVD_SPAN + CVD_PER * t, v);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if (lane == 0) wsum[wv] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t total = 0;
#pragma unroll
        for (uint32_t k = 0; k < CV_BLOCK / 64; k++) total += wsum[k];
        sums[blockIdx.x] = total;
    }
}

// arr[0..m) -> its exclusive prefix sums, in place, block b starting from base[b] (base null: one block, from zero,
// and *total = the sum).  A lane reads and writes its own CVD_PER entries only; the wave scan is cv_pmt_scan_kernel's.
__global__ __launch_bounds__(CV_BLOCK) void cv_dedupe_scan_kernel(uint32_t m, uint32_t *__restrict__ arr,
                                                                  const uint32_t *__restrict__ base,
                                                                  uint32_t *__restrict__ total) {
    __shared__ uint32_t wsum[CV_BLOCK / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * CVD_SPAN + CVD_PER * t;
    uint32_t v[CVD_PER];
    const uint32_t own = cvd_load(m, arr, i0, v);
    uint32_t inc = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d, 64);
        if ((int)lane >= d) inc += y;
    }
    if (lane == 63u) wsum[wv] = inc;
    __syncthreads();
    uint32_t run = (base ? base[blockIdx.x] : 0u) + inc - own;
#pragma unroll
    for (uint32_t k = 0; k < CV_BLOCK / 64; k++) run += k < wv ? wsum[k] : 0u;
#pragma unroll
    for (uint32_t q = 0; q < CVD_PER; q++) {
        if (i0 + q < m) arr[i0 + q] = run;
        run += v[q];
    }
    if (total && t == CV_BLOCK - 1) *total = run;   // the last lane's sum runs over the whole block
}
