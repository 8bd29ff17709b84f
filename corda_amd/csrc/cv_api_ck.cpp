// cv_api_ck.cpp — missing signers of the C-ABI (include/cordaverify.h): cv_missing_signers, its device-resident form
// and the workspace size.  The per-lane logic is cv_ck.h's; the engine state is cv_host.h's; the range checks, the
// buffer's layout and CvCk over it are cv_batch.h's.
#include "cv_batch.h"

using namespace cvh;

static_assert(CV_VS_OK == CVCK_VS_OK && CV_VS_BAD_SIGNATURE == CVCK_VS_BAD_SIGNATURE && CV_VS_MISSING == CVCK_VS_MISSING &&
                  CV_VS_MALFORMED == CVCK_VS_MALFORMED && CV_CK_LEAF == 0 && CV_CK_NODE == 1,
              "cv_ck.h and the public header agree");

extern "C" {

uint64_t cv_missing_signers_workspace(size_t ntx, size_t nnodes) { return cvck_ws_bytes(ntx, nnodes); }

int cv_missing_signers(cv_ctx *ctx, size_t ntx, size_t nreq, size_t nnodes, size_t nchild, size_t nsig,
                       const uint8_t *kind, const uint8_t *leaf_key, const int32_t *threshold,
                       const uint32_t *child_begin, const uint32_t *child, const int32_t *weight,
                       const uint32_t *req_begin, const uint32_t *tx_req_begin, const uint8_t *sig_key,
                       const uint32_t *tx_sig_begin, const uint8_t *req_allowed, const uint64_t *verdict_bitmap,
                       uint32_t wide_min, uint8_t *req_missing, uint8_t *tx_status) {
    if (ntx == 0) return CV_OK;
    if (ntx > 0xfffffffeull || nreq > 0xfffffffeull || nnodes > 0xfffffffeull || nchild > 0xfffffffeull ||
        nsig > 0xfffffffeull)
        return CV_E_TOO_LARGE;
    if (!req_begin || !tx_req_begin || !tx_sig_begin || !tx_status || (nreq && !req_missing)) return CV_E_ARGS;
    if (nnodes && (!kind || !leaf_key || !threshold || !child_begin)) return CV_E_ARGS;
    if ((nchild && (!child || !weight)) || (nsig && !sig_key)) return CV_E_ARGS;
    // the outer ranges must be well formed for the kernels to stay inside the buffers; child_begin's ends too — what
    // lies between them is checked per requirement on the device (CV_VS_MALFORMED fails one transaction, not the batch)
    if (!ranges_ok(tx_req_begin, ntx, nreq) || !ranges_ok(tx_sig_begin, ntx, nsig) || !ranges_ok(req_begin, nreq, nnodes))
        return CV_E_ARGS;
    if (nnodes ? (child_begin[0] != 0 || child_begin[nnodes] != nchild) : nchild != 0) return CV_E_ARGS;
    if (!ctx) return CV_E_ARGS;
    return dispatch_one(ctx, ntx, [&](Device &d, size_t, size_t, int) {
        CV_TRY(hipSetDevice(d.ordinal));
        const size_t nwords = (nsig + 63) / 64;
        Layout lay;
        const size_t o_kind = lay.take(nnodes), o_key = lay.take(32 * nnodes), o_thr = lay.take(4 * nnodes);
        const size_t o_cb = lay.take(4 * (nnodes + 1)), o_child = lay.take(4 * nchild), o_w = lay.take(4 * nchild);
        const size_t o_rb = lay.take(4 * (nreq + 1)), o_trb = lay.take(4 * (ntx + 1)), o_sig = lay.take(32 * nsig);
        const size_t o_tsb = lay.take(4 * (ntx + 1)), o_allow = lay.take(nreq), o_bm = lay.take(8 * nwords);
        const size_t o_miss = lay.take(nreq), o_st = lay.take(ntx), o_ws = lay.take((size_t)cvck_ws_bytes(ntx, nnodes));
        CV_TRY(d.ck.ensure(lay.top));
        uint8_t *base = d.ck.as<uint8_t>();
        hipStream_t s = d.stream;
        auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });
        auto up = [&](size_t off, const void *src, size_t bytes) {
            return bytes ? hipMemcpyAsync(base + off, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
        };
        CV_TRY(up(o_kind, kind, nnodes));
        CV_TRY(up(o_key, leaf_key, 32 * nnodes));
        CV_TRY(up(o_thr, threshold, 4 * nnodes));
        if (nnodes) CV_TRY(up(o_cb, child_begin, 4 * (nnodes + 1)));
        CV_TRY(up(o_child, child, 4 * nchild));
        CV_TRY(up(o_w, weight, 4 * nchild));
        CV_TRY(up(o_rb, req_begin, 4 * (nreq + 1)));
        CV_TRY(up(o_trb, tx_req_begin, 4 * (ntx + 1)));
        CV_TRY(up(o_sig, sig_key, 32 * nsig));
        CV_TRY(up(o_tsb, tx_sig_begin, 4 * (ntx + 1)));
        if (req_allowed) CV_TRY(up(o_allow, req_allowed, nreq));
        if (verdict_bitmap) CV_TRY(up(o_bm, verdict_bitmap, 8 * nwords));
        const CvCk a = ck_args(base, {ntx, nreq, nnodes, nchild, nsig},
                               {o_kind, o_key, o_thr, o_cb, o_child, o_w, o_rb, o_trb, o_sig, o_tsb, o_allow, o_bm, o_ws,
                                o_miss, o_st},
                               req_allowed != nullptr, verdict_bitmap != nullptr, wide_min);
        CV_TRY(cvk_ck(&a, s));
        if (nreq) CV_TRY(hipMemcpyAsync(req_missing, base + o_miss, nreq, hipMemcpyDeviceToHost, s));
        CV_TRY(hipMemcpyAsync(tx_status, base + o_st, ntx, hipMemcpyDeviceToHost, s));
        CV_TRY(hipStreamSynchronize(s));
        drain.armed = false;
        return CV_OK;
    });
}

int cv_missing_signers_device(cv_ctx *ctx, int device, size_t ntx, size_t nreq, size_t nnodes, size_t nchild, size_t nsig,
                              const void *d_kind, const void *d_leaf_key, const void *d_threshold,
                              const void *d_child_begin, const void *d_child, const void *d_weight,
                              const void *d_req_begin, const void *d_tx_req_begin, const void *d_sig_key,
                              const void *d_tx_sig_begin, const void *d_req_allowed, const void *d_bitmap,
                              uint32_t wide_min, void *d_req_missing, void *d_tx_status, void *d_workspace, void *stream) {
    if (!ctx) return CV_E_ARGS;
    if (ntx == 0) return CV_OK;
    if (ntx > 0xfffffffeull || nreq > 0xfffffffeull || nnodes > 0xfffffffeull || nchild > 0xfffffffeull ||
        nsig > 0xfffffffeull)
        return CV_E_TOO_LARGE;
    Device *d = find_dev(ctx, device);
    if (!d || !d_req_begin || !d_tx_req_begin || !d_tx_sig_begin || !d_tx_status || !d_workspace || (nreq && !d_req_missing))
        return CV_E_ARGS;
    if (nnodes && (!d_kind || !d_leaf_key || !d_threshold || !d_child_begin)) return CV_E_ARGS;
    if ((nchild && (!d_child || !d_weight)) || (nsig && !d_sig_key)) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(d->mu);
    CV_TRY(hipSetDevice(d->ordinal));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : d->stream;
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    CvCk a{};
    a.ntx = (uint32_t)ntx, a.nreq = (uint32_t)nreq, a.nnodes = (uint32_t)nnodes, a.nchild = (uint32_t)nchild;
    a.nsig = (uint32_t)nsig;
    a.kind = static_cast<const uint8_t *>(d_kind), a.leaf_key = static_cast<const uint8_t *>(d_leaf_key);
    a.threshold = static_cast<const int32_t *>(d_threshold), a.child_begin = static_cast<const uint32_t *>(d_child_begin);
    a.child = static_cast<const uint32_t *>(d_child), a.weight = static_cast<const int32_t *>(d_weight);
    a.req_begin = static_cast<const uint32_t *>(d_req_begin), a.tx_req_begin = static_cast<const uint32_t *>(d_tx_req_begin);
    a.sig_key = static_cast<const uint8_t *>(d_sig_key), a.tx_sig_begin = static_cast<const uint32_t *>(d_tx_sig_begin);
    a.req_allowed = static_cast<const uint8_t *>(d_req_allowed), a.bitmap = static_cast<const uint64_t *>(d_bitmap);
    a.wide_min = wide_min;
    a.count = reinterpret_cast<uint32_t *>(ws), a.list = reinterpret_cast<uint32_t *>(ws + CVCK_WS_LIST);
    a.flag = ws + cvck_ws_flag_off(ntx);
    a.req_missing = static_cast<uint8_t *>(d_req_missing), a.tx_status = static_cast<uint8_t *>(d_tx_status);
    CV_TRY(cvk_ck(&a, s));
    return CV_OK;
}

}  // extern "C"
