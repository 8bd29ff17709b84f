// cv_k_uniq.hip — the notary's uniqueness set (f4 / a11, the commit step): one kernel per step of cv_uniq.h.
// Shared helpers and every kernel declaration: cv_kcommon.h; launchers: cv_kernels.hip (cvk_uniq_*).
// No kernel here waits for another lane's store, and every probe loop is bounded by its table's slot count.
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
