// cv_k_notary.hip — the notary's fused commit step (a11, cv_notarise_batch): the kernels between the stages, one per
// step of cv_notary.h, and the scatter of the notary's signatures.  Shared helpers and every kernel declaration:
// cv_kcommon.h; launchers: cv_kernels.hip (cvk_notary_*).  No kernel here waits for another lane's store.
#include "cv_kcommon.h"

__global__ __launch_bounds__(CV_BLOCK) void cv_notary_gate_kernel(CvNotary N) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t < N.ntx) cvn_gate(N, t);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_notary_gather_kernel(CvNotary N) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < N.nstates) cvn_gather(N, i);
}

// ONE workgroup walks the batch in chunks of CVN_SCAN_BLOCK transactions, so the accepted list keeps the request
// order: a lane's place is the count of the chunks before (the same in every lane: each adds up the chunk's wave
// totals itself), of the waves before it in the chunk (LDS) and of the lanes before it in its wave (a ballot).
// count: the word that takes the list's length.
__global__ __launch_bounds__(CVN_SCAN_BLOCK) void cv_notary_final_kernel(CvNotary N, uint32_t *count) {
    constexpr uint32_t WAVES = CVN_SCAN_BLOCK / 64;
    __shared__ uint32_t wsum[WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < N.ntx; c0 += CVN_SCAN_BLOCK) {
        const uint32_t t = c0 + threadIdx.x;          // ntx <= 2^30 (the host's check): no wrap
        const bool acc = t < N.ntx && cvn_final(N, t) != 0;
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
        if (acc) cvn_place(N, t, base + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
        base += total;
        __syncthreads();                              // wsum is rewritten by the next chunk
    }
    if (threadIdx.x == 0) *count = base;
}

// signature j of the compact array goes to transaction list[j]: four lanes a signature, 16 bytes each
__global__ __launch_bounds__(CV_BLOCK) void cv_notary_scatter_kernel(uint32_t count, const uint32_t *__restrict__ list,
                                                                     const uint4 *__restrict__ sig,
                                                                     uint4 *__restrict__ out) {
    const uint32_t g = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (g < 4 * count) out[(size_t)list[g >> 2] * 4 + (g & 3u)] = sig[g];
}
