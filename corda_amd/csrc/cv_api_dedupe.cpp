// cv_api_dedupe.cpp — the device key dedupe of the C-ABI (include/cordaverify.h): cv_ed25519_dedupe_keys_device and its
// workspace size.  The steps and the workspace's layout are cv_keydedupe.h's; the engine state is cv_host.h's.  The
// fused batch calls reach the same launcher through cv_batch.h's FusedKeyed.
#include "cv_host.h"

using namespace cvh;

extern "C" {

int cv_ed25519_dedupe_keys_device(cv_ctx *ctx, int device, size_t n, const void *d_pk, void *d_keys, void *d_key_index,
                                  void *d_nkeys, void *d_workspace, void *stream) {
    // the checks that need no device first
    if (n == 0) return CV_OK;
    if (n > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (!ctx) return CV_E_ARGS;
    Device *d = find_dev(ctx, device);
    if (!d || !d_pk || !d_keys || !d_key_index || !d_nkeys || !d_workspace) return CV_E_ARGS;
    const CvdLayout L = cvd_layout(n);
    const CvDedupe D = cvd_args(n, d_pk, d_keys, d_key_index, d_nkeys, d_workspace, key_seed(1) | 1, L);
    uint8_t *w = static_cast<uint8_t *>(d_workspace);
    uint32_t *sums[CVD_LEVELS];
    for (int k = 0; k < CVD_LEVELS; k++) sums[k] = reinterpret_cast<uint32_t *>(w + L.sum[k]);
    std::lock_guard<std::mutex> g(d->mu);              // enqueue only
    CV_TRY(hipSetDevice(d->ordinal));
    CV_TRY(cvk_dedupe(&D, sums, stream ? static_cast<hipStream_t>(stream) : d->stream));
    return CV_OK;
}

uint64_t cv_ed25519_dedupe_keys_workspace(size_t n) { return n > 0xfffffffeull ? 0 : cvd_layout(n).bytes; }

}  // extern "C"
