// cv_api_hotkeys.cpp — the hot-key route of the C-ABI (include/cordaverify.h):
// cv_ed25519_verify_device_hotkeys, its workspace size, and the two halves the fused batch calls share with it through
// cv_host.h — hotkeys_front (what runs before the route's one read-back) and verify_hotkeys_locked (the decision and
// what runs behind it).  The steps and the workspace's layout are cv_hotkeys.h's; the engine state is cv_host.h's.
#include "cv_host.h"

using namespace cvh;

// The dedupe, then tally .. the records' scan, then the copy of head | `rows` hot key rows to `host` (pinned, or
// pageable memory that outlives the caller's synchronisation).  Enqueue only.
hipError_t cvh::hotkeys_front(const CvHot &H, const CvhLayout &L, void *ws, uint64_t seed, size_t rows, void *host,
                              hipStream_t s) {
    uint8_t *w = static_cast<uint8_t *>(ws);
    const CvDedupe D = cvh_dedupe_args(H.n, H.pk, ws, seed, L);
    uint32_t *sums[CVD_LEVELS];
    for (int k = 0; k < CVD_LEVELS; k++) sums[k] = reinterpret_cast<uint32_t *>(w + L.dedupe + L.D.sum[k]);
    hipError_t e = cvk_dedupe(&D, sums, s);
    if (e == hipSuccess) e = cvk_hotkeys_front(&H, sums, s);
    if (e == hipSuccess) e = hipMemcpyAsync(host, H.head, 4 * CVH_HEAD_WORDS + 32 * rows, hipMemcpyDeviceToHost, s);
    return e;
}

// Behind the read-back: no hot key — the unkeyed launch group over the caller's arrays into the caller's outputs;
// every key hot — the keyed one with the dedupe's own numbering (hot numbering equals key numbering then); else the
// gather, the keyed group over rows [0, nhot), the unkeyed one over rows [nhot, n), and the merge.
int cvh::verify_hotkeys_locked(cv_ctx *ctx, Device &d, const CvHot &H, size_t rows, const void *host, const uint8_t *arena,
                               uint64_t *bitmap, uint8_t *status, hipStream_t s, uint32_t route_out[4]) {
    const uint32_t *head = static_cast<const uint32_t *>(host);
    const uint8_t *hrows = static_cast<const uint8_t *>(host) + 4 * CVH_HEAD_WORDS;
    const uint32_t n = H.n, nk = head[CVH_HEAD_NKEYS], hk = head[CVH_HEAD_HOTKEYS], nhot = head[CVH_HEAD_NHOT];
    if (!head[CVH_HEAD_OK] || nk == 0 || nk > n || hk > nk || hk > rows || nhot > n || (hk == 0) != (nhot == 0) ||
        (hk == nk) != (nhot == n))
        return CV_E_HIP;
    if (route_out) route_out[0] = nk, route_out[1] = hk, route_out[2] = nhot, route_out[3] = n - nhot;
    const uint8_t *pk = reinterpret_cast<const uint8_t *>(H.pk), *sig = reinterpret_cast<const uint8_t *>(H.sig);
    if (hk == 0) return hip_rc(verify_device_locked(ctx, d, n, pk, sig, arena, H.off, H.len, bitmap, status, s));
    if (hk == nk)
        return verify_keyed_locked(ctx, d, n, nk, hrows, reinterpret_cast<const uint8_t *>(H.keys), H.key_index, sig, arena,
                                   H.off, H.len, bitmap, status, s, nullptr);
    CV_TRY(cvk_hotkeys_gather(&H, s));
    uint8_t *sub = status ? const_cast<uint8_t *>(H.sub_status) : nullptr;
    const int rc = verify_keyed_locked(ctx, d, nhot, hk, hrows, reinterpret_cast<const uint8_t *>(H.hot_keys), H.g_kidx,
                                       reinterpret_cast<const uint8_t *>(H.g_sig), arena, H.g_off, H.g_len,
                                       const_cast<uint64_t *>(H.bm_hot), sub, s, nullptr);
    if (rc != CV_OK) return rc;
    CV_TRY(verify_device_locked(ctx, d, n - nhot, reinterpret_cast<const uint8_t *>(H.g_pk) + 32 * (size_t)nhot,
                                reinterpret_cast<const uint8_t *>(H.g_sig) + 64 * (size_t)nhot, arena, H.g_off + nhot,
                                H.g_len + nhot, const_cast<uint64_t *>(H.bm_cold), sub ? sub + nhot : nullptr, s));
    CV_TRY(cvk_hotkeys_merge(&H, bitmap, status, s));
    return CV_OK;
}

extern "C" {

int cv_ed25519_verify_device_hotkeys(cv_ctx *ctx, int device, size_t n, const void *d_pk, const void *d_sig,
                                     const void *d_arena, const void *d_off, const void *d_len, void *d_bitmap,
                                     void *d_status, uint32_t hot_min, void *d_workspace, void *stream,
                                     uint32_t route_out[4]) {
    // the checks that need no device first
    if (n == 0) return CV_OK;
    if (n > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (!ctx) return CV_E_ARGS;
    Device *d = find_dev(ctx, device);
    if (!d || !d_pk || !d_sig || !d_arena || !d_off || !d_len || !d_bitmap || !d_workspace) return CV_E_ARGS;
    const uint32_t cap = ctx->key_cap.load();
    const CvhLayout L = cvh_layout(n);
    const CvHot H = cvh_args(n, hot_min, cap, d_pk, d_sig, d_off, d_len, d_workspace, L);
    const size_t rows = (size_t)cvh_rows(n, H.hot_min, cap);
    std::vector<uint32_t> host(CVH_HEAD_WORDS + 8 * rows);
    std::lock_guard<std::mutex> g(d->mu);
    CV_TRY(hipSetDevice(d->ordinal));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : d->stream;
    hipError_t e = hotkeys_front(H, L, d_workspace, key_seed(1) | 1, rows, host.data(), s);
    const hipError_t e2 = hipStreamSynchronize(s);     // the one synchronisation; also on an error: `host` is leaving
    CV_TRY(e);
    CV_TRY(e2);
    return verify_hotkeys_locked(ctx, *d, H, rows, host.data(), static_cast<const uint8_t *>(d_arena),
                                 static_cast<uint64_t *>(d_bitmap), static_cast<uint8_t *>(d_status), s, route_out);
}

uint64_t cv_ed25519_verify_hotkeys_workspace(size_t n) { return n > 0xfffffffeull ? 0 : cvh_layout(n).bytes; }

}  // extern "C"
