// cv_k_tearoff.hip — the verifier side of a tear-off (f3, cv_filtered_verify) and the oracle's signing step fused
// around it (cv_tearoff_sign_batch): the kernels between the stages, one per step of cv_tearoff.h.  The leaf hashes,
// the tree verify, the signing and the scatter of the signatures are the existing kernels.  Shared helpers and every
// kernel declaration: cv_kcommon.h; launchers: cv_kernels.hip (cvk_tearoff_*).  No kernel here waits for another
// lane's store.
#include "cv_kcommon.h"

__global__ __launch_bounds__(CV_BLOCK) void cv_tearoff_check_kernel(CvTearoff T) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < T.nleaves) cvt_check(T, i);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_tearoff_gate_kernel(CvTearoff T) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t < T.ntx) cvt_gate(T, t);
}

// ONE workgroup walks the batch in chunks of CVT_SCAN_BLOCK tear-offs, so the accepted list keeps the request order
// (the structure of cv_notary_final_kernel): a lane's place is the count of the chunks before (the same in every
// lane: each adds up the chunk's wave totals itself), of the waves before it in the chunk (LDS) and of the lanes
// before it in its wave (a ballot).  count: the word that takes the list's length.
__global__ __launch_bounds__(CVT_SCAN_BLOCK) void cv_tearoff_compact_kernel(CvTearoff T, uint32_t *count) {
    constexpr uint32_t WAVES = CVT_SCAN_BLOCK / 64;
    __shared__ uint32_t wsum[WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < T.ntx; c0 += CVT_SCAN_BLOCK) {
        const uint32_t t = c0 + threadIdx.x;          // c0 < ntx <= 0xfffffffe: t >= c0 unless it wrapped
        const bool acc = t >= c0 && t < T.ntx && cvt_accepted(T, t) != 0;
        const unsigned long long m = __ballot(acc);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < WAVES; w++) {
            const uint32_t v = wsum[w];
            before += w < wave ? v : 0u;
            total += v;
        }
        if (acc) cvt_place(T, t, base + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
        base += total;
        __syncthreads();                              // wsum is rewritten by the next chunk
        if (c0 + CVT_SCAN_BLOCK < c0) break;          // the last chunk below 2^32
    }
    if (threadIdx.x == 0) *count = base;
}
