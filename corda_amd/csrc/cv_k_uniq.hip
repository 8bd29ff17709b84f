// cv_k_uniq.hip — the notary's uniqueness set (f4 / a11, the commit step): one kernel per step of cv_uniq.h.
// Shared helpers and every kernel declaration: cv_kcommon.h; launchers: cv_kernels.hip (cvk_uniq_*).
// No kernel here waits for another lane's store, and every probe loop is bounded by its table's slot count.  The
// snapshot's kernels meet their block at one barrier each, which every lane reaches.
#include "cv_kcommon.h"

// the sum of v over the wave's lanes, in lane 0 (every lane of the wave calls it)
static __device__ __forceinline__ uint32_t cvu_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

__global__ __launch_bounds__(CV_BLOCK) void cv_uniq_init_kernel(CvUniqBatch B, uint32_t *__restrict__ stat) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t < B.ntx) cvu_init(B, stat, t);
}

// one lane per state; stat == null for cv_uniq_load's check
__global__ __launch_bounds__(CV_BLOCK) void cv_uniq_group_kernel(CvUniqTable T, CvUniqBatch B, uint32_t *stat) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < B.nstates) cvu_group(T, B, stat, i);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_uniq_claim_kernel(CvUniqBatch B, const uint32_t *__restrict__ stat) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t < B.ntx) cvu_claim(B, stat, t);
}

// undecided: the round's word of the counters, one atomic per wave that still holds an undecided request
__global__ __launch_bounds__(CV_BLOCK) void cv_uniq_decide_kernel(CvUniqBatch B, const uint32_t *__restrict__ stat_in,
                                                                  uint32_t *__restrict__ stat_out, uint32_t *undecided) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    const uint32_t u = cvu_wave_sum(t < B.ntx ? cvu_decide(B, stat_in, stat_out, t) : 0u);
    if ((threadIdx.x & 63u) == 0 && u) atomicAdd(undecided, u);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_uniq_own_kernel(CvUniqBatch B, const uint32_t *__restrict__ stat) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t < B.ntx) cvu_own(B, stat, t);
}

// The serial tail: ONE wave.  Its lanes read 64 statuses at a time; lane 0 alone decides the undecided ones among
// them, in ascending order (the ballot is uniform, so the loop is too).  Nothing here waits: lanes 1..63 only load.
__global__ __launch_bounds__(64) void cv_uniq_tail_kernel(CvUniqBatch B, uint32_t *stat) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t base = 0; base < B.ntx; base += 64) {
        const uint32_t t = base + lane;
        unsigned long long m = __ballot(t < B.ntx && stat[t] == CVU_UNDECIDED);
        if (lane == 0) {
            while (m) {
                const uint32_t k = (uint32_t)__ffsll((long long)m) - 1u;
                m &= m - 1;
                cvu_tail_one(B, stat, base + k);
            }
        }
    }
}

__global__ __launch_bounds__(CV_BLOCK) void cv_uniq_report_kernel(CvUniqTable T, CvUniqBatch B, const uint32_t *stat) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    const uint32_t put = cvu_wave_sum(t < B.ntx ? cvu_report(T, B, stat, t) : 0u);
    if ((threadIdx.x & 63u) == 0 && put) atomicAdd(B.dstat + CVU_D_INSERTED, put);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_uniq_load_check_kernel(CvUniqBatch B) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < B.nstates) cvu_load_check(B, i);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_uniq_load_put_kernel(CvUniqTable T, CvUniqBatch B) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < B.nstates) cvu_load_put(T, B, i);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_uniq_lookup_kernel(CvUniqTable T, uint32_t n, const uint32_t *__restrict__ key,
                                                                  uint8_t *__restrict__ found, uint32_t *__restrict__ cons_id,
                                                                  uint32_t *__restrict__ cons_index,
                                                                  uint32_t *__restrict__ cons_caller, uint32_t *dstat) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < n) cvu_lookup(T, key, i, found, cons_id, cons_index, cons_caller, dstat);
}

// growth: one lane per slot of the old table (from.mask + 1 of them)
__global__ __launch_bounds__(CV_BLOCK) void cv_uniq_rehash_kernel(CvUniqTable from, CvUniqTable to, uint32_t *dstat) {
    const uint64_t s = (uint64_t)blockIdx.x * CV_BLOCK + threadIdx.x;
    if (s <= from.mask) cvu_rehash(from, to, (uint32_t)s, dstat);
}

// ---- snapshot (cv_uniq.h): one lane per slot of the window, CV_BLOCK slots a block
// the lane's flag -> (occupied slots in the lanes of the block before this one, the block's total when `total`)
static __device__ __forceinline__ uint32_t cvu_block_rank(bool occ, uint32_t *wsum, uint32_t *total) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(occ);
    if (lane == 0) wsum[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
    for (uint32_t k = 0; k < CV_BLOCK / 64; k++) {
        before += k < wv ? wsum[k] : 0u;
        all += wsum[k];
    }
    if (total) *total = all;
    return before;
}

__global__ __launch_bounds__(CV_BLOCK) void cv_uniq_snap_count_kernel(CvUniqTable T, CvUniqSnap S, uint32_t *__restrict__ sums) {
    __shared__ uint32_t wsum[CV_BLOCK / 64];
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    uint32_t total = 0;
    (void)cvu_block_rank(cvu_snap_occupied(T, S, i) != 0, wsum, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// base: the scanned block totals.  A wave's occupied lanes hold consecutive ranks, so their records are adjacent.
__global__ __launch_bounds__(CV_BLOCK) void cv_uniq_snap_emit_kernel(CvUniqTable T, CvUniqSnap S, const uint32_t *__restrict__ base) {
    __shared__ uint32_t wsum[CV_BLOCK / 64];
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    const bool occ = cvu_snap_occupied(T, S, i) != 0;
    const uint32_t rank = base[blockIdx.x] + cvu_block_rank(occ, wsum, nullptr);
    if (occ) cvu_snap_emit(T, S, i, rank);
    if (i == 0) cvu_snap_close(S);
}
