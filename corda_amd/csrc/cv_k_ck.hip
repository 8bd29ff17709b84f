// cv_k_ck.hip — missing signers (CompositeKey fulfilment) of a batch: the narrow and the wide kernel around the
// per-lane core of cv_ck.h.  Kernel declarations: cv_kcommon.h; launcher: cv_kernels.hip (cvk_ck).
#include "cv_kcommon.h"
#include "cv_ck.h"

// One lane per transaction: decides it (req_missing of its requirements, tx_status) or, at or above wide_min,
// appends it to the list for the wide kernel.  The list's counter was cleared on the stream before the launch.
__global__ __launch_bounds__(CV_BLOCK) void cv_ck_narrow_kernel(CvCk C) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t >= C.ntx) return;
    cvck_narrow_tx(C, t);
}

// One wave per listed transaction; a workgroup IS one wave, so the barrier between two phases is the workgroup's and
// every loop around it runs the same number of times on all its lanes (t, and so the tile count, is the wave's).
// The grid is fixed and strides over the list, whose length is read from device memory: no host read-back.
__global__ __launch_bounds__(64) void cv_ck_wide_kernel(CvCk C) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[CV_CK_TILE * 32];
    const uint32_t lane = threadIdx.x;
    const uint32_t listed = *C.count < C.ntx ? *C.count : C.ntx;
    for (uint32_t i = blockIdx.x; i < listed; i += gridDim.x) {
        const uint32_t t = C.list[i];
        if (t >= C.ntx) continue;                   // (cannot happen: the narrow kernel wrote the entry)
        cvck_wide_clear(C, t, lane);
        const uint32_t tiles = cvck_tiles(C, t);
        for (uint32_t j = 0; j < tiles; j++) {
            __syncthreads();                        // the previous tile's readers are done
            cvck_wide_stage(C, t, j, lane, tile);
            __syncthreads();
            cvck_wide_match(C, t, j, lane, tile);
        }
        __syncthreads();                            // the Leaf flags are written
        const uint32_t bits = cvck_wide_reqs(C, t, lane);
        uint32_t all = 0;
        if (__ballot(bits & CVCK_M_MALFORMED)) all |= CVCK_M_MALFORMED;
        if (__ballot(bits & CVCK_M_BADSIG)) all |= CVCK_M_BADSIG;
        if (__ballot(bits & CVCK_M_NEEDED)) all |= CVCK_M_NEEDED;
        if (lane == 0) C.tx_status[t] = cvck_status(all, C.tx_sig_begin[t + 1] - C.tx_sig_begin[t]);
        __syncthreads();                            // the tile is free for the next transaction
    }
}
