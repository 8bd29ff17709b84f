// cv_k_resolve.hip — the graph kernels of cv_resolve_batch (f1, ResolveTransactionsFlow): one per step of
// cv_resolve.h — the join table's insert (a lane per transaction), its probe (a lane per input) and the gate (a lane
// per transaction).  Shared helpers and every kernel declaration: cv_kcommon.h; launchers: cv_kernels.hip
// (cvk_resolve_*).  No kernel here waits for another lane's store; the kernel boundaries publish the table and the
// input statuses.
#include "cv_kcommon.h"

__global__ __launch_bounds__(CV_BLOCK) void cv_resolve_insert_kernel(CvResolve R) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t < R.ntx) cvr_insert(R, t);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_resolve_probe_kernel(CvResolve R) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < R.ninputs) cvr_probe(R, i);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_resolve_gate_kernel(CvResolve R) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t < R.ntx) cvr_gate(R, t);
}
