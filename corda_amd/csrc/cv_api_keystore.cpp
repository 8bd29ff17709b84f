// cv_api_keystore.cpp — the device key store of the C-ABI (include/cordaverify.h): the cv_keystore_* entry points and
// cv_sign_transactions.  The engine state and the resident frame are cv_host.h's; the range checks and the layout of a
// call's workspace are cv_batch.h's; the per-lane core is cv_keystore.h.
#include "cv_batch.h"

using namespace cvh;

// The key store: a resident frame (cv_host.h) whose table is occ | rec (cv_keystore.h), overwritten before it is
// freed, with a pinned staging block for the seeds.
struct cv_keystore : Resident {
    CvKeyTable T{};
    PinBuf pin;                              // the seeds on their way up; wiped before cv_keystore_add returns
};

namespace {

void wipe(volatile uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; i++) p[i] = 0;
}

}  // namespace

extern "C" {

int cv_keystore_open(cv_ctx *ctx, int device, size_t capacity_keys, cv_keystore **out) {
    int rc = Resident::open_check(ctx, device, capacity_keys, out);
    if (rc != CV_OK) return rc;
    std::unique_ptr<cv_keystore> ks(new (std::nothrow) cv_keystore());
    if (!ks) return CV_E_OOM;
    std::random_device rd;
    const uint64_t seed = key_seed(2) ^ rand64(rd);
    rc = ks->open(ctx, device, capacity_keys, CKS_SLOT_BYTES, CKS_D_WORDS, true);   // tables overwritten before freed
    if (rc != CV_OK) {
        cv_keystore_close(ks.release());
        return rc;
    }
    ks->T = cks_carve(ks->tab, ks->slots, seed);
    *out = ks.release();
    return CV_OK;
}

void cv_keystore_close(cv_keystore *ks) {
    if (!ks) return;
    ks->close([ks] { ks->pin.release(); });
    delete ks;
}

int cv_keystore_reserve(cv_keystore *ks, size_t capacity_keys) {
    if (!ks) return CV_E_ARGS;
    if (capacity_keys > kUniqMaxStates) return CV_E_TOO_LARGE;
    std::lock_guard<std::mutex> g(ks->mu);
    CvKeyTable to{};
    bool rehashed = false;
    const int rc = ks->grow(
        capacity_keys,
        [&](void *base, size_t slots) {
            to = cks_carve(base, slots, ks->T.seed);
            return cvk_ks_rehash(&ks->T, &to, ks->dstat.as<uint32_t>(), ks->stream);
        },
        [ks] { return ks->stat_end(); }, &rehashed);
    if (rehashed) ks->T = to;
    return rc;
}

int cv_keystore_stats(cv_keystore *ks, uint64_t *out, size_t nout) {
    if (!ks || (nout && !out)) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(ks->mu);
    const uint64_t v[CV_KS_STAT_COUNT] = {ks->resident, ks->capacity, (uint64_t)ks->slots, ks->last_probe};
    for (size_t k = 0; k < nout; k++) out[k] = k < CV_KS_STAT_COUNT ? v[k] : 0;
    return CV_OK;
}

int cv_keystore_add(cv_keystore *ks, size_t n, const uint8_t *seed, uint8_t *pk_out, uint8_t *status) {
    if (n == 0) return CV_OK;
    if (n > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (!seed || !pk_out || !status) return CV_E_ARGS;
    if (n > kUniqMaxStates) return CV_E_TOO_LARGE;
    if (!ks) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(ks->mu);
    if (ks->resident + n > ks->capacity) return CV_E_OOM;        // before any change and any output
    CV_TRY(hipSetDevice(ks->ordinal));
    // seeds | staged records | pk | status | the call-local table with its stat behind it, first, number
    const CvdLayout L = cvd_layout(n);
    Layout lay;
    const size_t o_seed = lay.take(32 * n), o_rec = lay.take(4 * CKS_REC_WORDS * n), o_pk = lay.take(32 * n);
    const size_t o_st = lay.take(n), o_dd = lay.take((size_t)L.bytes);
    CV_TRY(ks->ws.ensure(lay.top + 16));
    CV_TRY(ks->pin.ensure(32 * n));
    uint8_t *base = ks->ws.as<uint8_t>(), *pin = ks->pin.as<uint8_t>();
    hipStream_t s = ks->stream;
    // whatever way the call ends: the stream drained, then the pinned seeds wiped
    auto drain = on_exit([s, pin, n] {
        (void)hipStreamSynchronize(s);
        wipe(pin, 32 * n);
    });
    std::memcpy(pin, seed, 32 * n);
    CV_TRY(hipMemcpyAsync(base + o_seed, pin, 32 * n, hipMemcpyHostToDevice, s));
    int rc = ks->stat_begin();
    if (rc != CV_OK) return rc;
    const CvDedupe D = cvd_args(n, base + o_pk, nullptr, nullptr, nullptr, base + o_dd, key_seed(3) | 1, L);
    hipError_t e = cvk_ks_add(&ks->T, &D, base + o_seed, at<uint32_t>(base, o_rec), base + o_st, ks->dstat.as<uint32_t>(), s);
    // the staged records hold a and prefix: cleared behind the put, also when a launch failed
    const hipError_t e2 = hipMemsetAsync(base + o_seed, 0, o_pk - o_seed, s);
    if (e == hipSuccess) e = e2;
    CV_TRY(e);
    rc = ks->stat_end();
    if (rc != CV_OK) return rc;
    ks->resident += ks->hstat[CKS_D_ADDED];                      // the store's extra
    CV_TRY(hipMemcpyAsync(pk_out, base + o_pk, 32 * n, hipMemcpyDeviceToHost, s));
    CV_TRY(hipMemcpyAsync(status, base + o_st, n, hipMemcpyDeviceToHost, s));
    CV_TRY(hipStreamSynchronize(s));
    return CV_OK;
}

int cv_keystore_contains(cv_keystore *ks, size_t n, const uint8_t *pk, uint8_t *found) {
    if (n == 0) return CV_OK;
    if (n > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (!pk || !found) return CV_E_ARGS;
    if (n > kUniqMaxStates) return CV_E_TOO_LARGE;
    if (!ks) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(ks->mu);
    CV_TRY(hipSetDevice(ks->ordinal));
    Layout lay;
    const size_t o_pk = lay.take(32 * n), o_f = lay.take(n);
    CV_TRY(ks->ws.ensure(lay.top + 16));
    uint8_t *base = ks->ws.as<uint8_t>();
    hipStream_t s = ks->stream;
    auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });   // the pageable copies read the caller's arrays
    CV_TRY(hipMemcpyAsync(base + o_pk, pk, 32 * n, hipMemcpyHostToDevice, s));
    int rc = ks->stat_begin();
    if (rc != CV_OK) return rc;
    CV_TRY(cvk_ks_lookup(&ks->T, (uint32_t)n, at<uint32_t>(base, o_pk), nullptr, base + o_f, 1, ks->dstat.as<uint32_t>(), s));
    rc = ks->stat_end();
    if (rc != CV_OK) return rc;
    CV_TRY(hipMemcpyAsync(found, base + o_f, n, hipMemcpyDeviceToHost, s));
    CV_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    return CV_OK;
}

int cv_keystore_sign(cv_keystore *ks, size_t n, const uint8_t *pk, const uint8_t *msg_arena, uint64_t msg_arena_bytes,
                     const uint64_t *msg_off, const uint32_t *msg_len, uint8_t *sig_out, uint8_t *status) {
    if (n == 0) return CV_OK;
    if (n > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (!pk || !msg_off || !msg_len || !sig_out || !status) return CV_E_ARGS;
    if (n > kUniqMaxStates) return CV_E_TOO_LARGE;
    // the messages' extent: a record past the arena, or one whose off + len wraps, fails before any copy or launch
    const Extent ext = arena_extent(0, n, msg_off, msg_len, msg_arena_bytes);
    const uint64_t lo = ext.lo, hi = ext.hi;
    if (!ext.ok || (hi > lo && !msg_arena)) return CV_E_ARGS;
    if (!ks) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(ks->mu);
    CV_TRY(hipSetDevice(ks->ordinal));
    Layout lay;
    const size_t o_pk = lay.take(32 * n), o_off = lay.take(8 * n), o_len = lay.take(4 * n), o_ar = lay.take(hi - lo);
    const size_t o_slot = lay.take(4 * n), o_st = lay.take(n), o_sig = lay.take(64 * n);
    CV_TRY(ks->ws.ensure(lay.top + 16));
    uint8_t *base = ks->ws.as<uint8_t>();
    hipStream_t s = ks->stream;
    auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });   // the pageable copies read the caller's arrays
    CV_TRY(hipMemcpyAsync(base + o_pk, pk, 32 * n, hipMemcpyHostToDevice, s));
    CV_TRY(hipMemcpyAsync(base + o_off, msg_off, 8 * n, hipMemcpyHostToDevice, s));
    CV_TRY(hipMemcpyAsync(base + o_len, msg_len, 4 * n, hipMemcpyHostToDevice, s));
    if (hi > lo) CV_TRY(hipMemcpyAsync(base + o_ar, msg_arena + lo, hi - lo, hipMemcpyHostToDevice, s));
    int rc = ks->stat_begin();
    if (rc != CV_OK) return rc;
    CV_TRY(cvk_ks_lookup(&ks->T, (uint32_t)n, at<uint32_t>(base, o_pk), at<uint32_t>(base, o_slot), base + o_st, CV_KS_OK,
                         ks->dstat.as<uint32_t>(), s));
    // the offsets are the caller's: the arena pointer is moved back by the part that was not copied
    CV_TRY(cvk_ks_sign(&ks->T, (uint32_t)n, at<uint32_t>(base, o_slot), base + o_ar - lo, at<uint64_t>(base, o_off),
                       at<uint32_t>(base, o_len), base + o_sig, s));
    rc = ks->stat_end();
    if (rc != CV_OK) return rc;
    CV_TRY(hipMemcpyAsync(sig_out, base + o_sig, 64 * n, hipMemcpyDeviceToHost, s));
    CV_TRY(hipMemcpyAsync(status, base + o_st, n, hipMemcpyDeviceToHost, s));
    CV_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    return CV_OK;
}

int cv_sign_transactions(cv_ctx *ctx, cv_keystore *ks, size_t ntx, const uint8_t *leaf_arena, uint64_t leaf_arena_bytes,
                         const uint64_t *leaf_off, const uint32_t *leaf_len, const uint32_t *tx_leaf_begin, size_t nsig,
                         const uint8_t *pk, const uint32_t *tx_sig_begin, uint8_t *tx_status, uint8_t *ids,
                         uint8_t *sig_out, uint32_t *first_bad) {
    if (ntx == 0) return CV_OK;
    if (ntx > 0xfffffffeull || nsig > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (!tx_leaf_begin || !tx_sig_begin || !tx_status || !ids) return CV_E_ARGS;
    if (!ranges_ok(tx_leaf_begin, ntx) || !ranges_ok(tx_sig_begin, ntx, nsig)) return CV_E_ARGS;
    const size_t T = ntx, L = tx_leaf_begin[ntx], N = nsig;
    if (L > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (L && (!leaf_off || !leaf_len)) return CV_E_ARGS;
    if (N && (!pk || !sig_out)) return CV_E_ARGS;
    if (T > kUniqMaxStates || L > kUniqMaxStates || N > kUniqMaxStates) return CV_E_TOO_LARGE;
    // the leaves' extent: a record past the arena, or one whose off + len wraps, fails before any copy or launch
    const Extent ext = arena_extent(0, L, leaf_off, leaf_len, leaf_arena_bytes);
    const uint64_t lo = ext.lo, hi = ext.hi;
    if (!ext.ok || (hi > lo && !leaf_arena)) return CV_E_ARGS;
    if (!ctx || !ks || ks->ctx != ctx) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(ks->mu);
    CV_TRY(hipSetDevice(ks->ordinal));
    // inputs | workspace | outputs
    Layout lay;
    const size_t i_arena = lay.take(hi - lo), i_loff = lay.take(8 * L), i_llen = lay.take(4 * L);
    const size_t i_txb = lay.take(4 * (T + 1)), i_tsb = lay.take(4 * (T + 1)), i_pk = lay.take(32 * N);
    const size_t w_ldig = lay.take(32 * L), w_slot = lay.take(4 * N), w_soff = lay.take(8 * N), w_slen = lay.take(4 * N);
    const size_t o_st = lay.take(T), o_ids = lay.take(32 * T), o_fb = lay.take(4 * T), o_sig = lay.take(64 * N);
    CV_TRY(ks->ws.ensure(lay.top + 16));
    uint8_t *base = ks->ws.as<uint8_t>();
    hipStream_t s = ks->stream;
    auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });   // the pageable copies read the caller's arrays
    if (hi > lo) CV_TRY(hipMemcpyAsync(base + i_arena, leaf_arena + lo, hi - lo, hipMemcpyHostToDevice, s));
    if (L) {
        CV_TRY(hipMemcpyAsync(base + i_loff, leaf_off, 8 * L, hipMemcpyHostToDevice, s));
        CV_TRY(hipMemcpyAsync(base + i_llen, leaf_len, 4 * L, hipMemcpyHostToDevice, s));
    }
    CV_TRY(hipMemcpyAsync(base + i_txb, tx_leaf_begin, 4 * (T + 1), hipMemcpyHostToDevice, s));
    CV_TRY(hipMemcpyAsync(base + i_tsb, tx_sig_begin, 4 * (T + 1), hipMemcpyHostToDevice, s));
    if (N) CV_TRY(hipMemcpyAsync(base + i_pk, pk, 32 * N, hipMemcpyHostToDevice, s));
    int rc = ks->stat_begin();
    if (rc != CV_OK) return rc;
    // the ids: leaf hashes, then the trees; they stay where the signing kernel reads them as its messages
    CV_TRY(cvk_merkle((uint32_t)T, (uint32_t)L, 0, base + i_arena - lo, at<uint64_t>(base, i_loff), at<uint32_t>(base, i_llen),
                      at<uint32_t>(base, i_txb), at<uint32_t>(base, w_ldig), base + o_ids, nullptr, s));
    CvKeyTx X{};
    X.ntx = (uint32_t)T;
    X.leaf_begin = at<uint32_t>(base, i_txb), X.sig_begin = at<uint32_t>(base, i_tsb), X.pk = at<uint32_t>(base, i_pk);
    X.slot = at<uint32_t>(base, w_slot), X.off = at<uint64_t>(base, w_soff), X.len = at<uint32_t>(base, w_slen);
    X.tx_status = base + o_st, X.first_bad = at<uint32_t>(base, o_fb);
    X.dstat = ks->dstat.as<uint32_t>();
    CV_TRY(cvk_ks_tx_gate(&ks->T, &X, s));
    CV_TRY(cvk_ks_sign(&ks->T, (uint32_t)N, X.slot, base + o_ids, X.off, X.len, base + o_sig, s));
    rc = ks->stat_end();
    if (rc != CV_OK) return rc;
    CV_TRY(hipMemcpyAsync(tx_status, base + o_st, T, hipMemcpyDeviceToHost, s));
    CV_TRY(hipMemcpyAsync(ids, base + o_ids, 32 * T, hipMemcpyDeviceToHost, s));
    if (first_bad) CV_TRY(hipMemcpyAsync(first_bad, base + o_fb, 4 * T, hipMemcpyDeviceToHost, s));
    if (N) CV_TRY(hipMemcpyAsync(sig_out, base + o_sig, 64 * N, hipMemcpyDeviceToHost, s));
    CV_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    return CV_OK;
}

}  // extern "C"
