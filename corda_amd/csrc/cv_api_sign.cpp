// cv_api_sign.cpp — signing entry points of the C-ABI (include/cordaverify.h): cv_ed25519_sign_batch (a seed per
// message), the fixed-key signer (cv_signer_*, cv_ed25519_sign_keyed) and their device-resident forms.  The engine
// state is cv_host.h's; the signer's record for a device is cv_batch.h's.
#include "cv_batch.h"

using namespace cvh;

extern "C" {

// ---------------------------------------------------------------- sign (host buffers)
static int sign_shard(Device &d, size_t b, size_t e, const uint8_t *seed, const uint8_t *arena, const uint64_t *off,
                      const uint32_t *len, uint8_t *pk, uint8_t *sig) {
    const size_t n = e - b;
    if (n == 0) return CV_OK;
    if (n > 0xffffffffull) return CV_E_TOO_LARGE;
    CV_TRY(hipSetDevice(d.ordinal));
    uint64_t lo = UINT64_MAX, hi = 0;
    for (size_t i = b; i < e; i++) {
        lo = std::min<uint64_t>(lo, off[i]);
        hi = std::max<uint64_t>(hi, off[i] + len[i]);
    }
    if (hi < lo) hi = lo;
    CV_TRY(d.seed.ensure(n * 32));
    CV_TRY(d.arena.ensure(hi - lo + 16));
    CV_TRY(d.off.ensure(n * 8));
    CV_TRY(d.len.ensure(n * 4));
    CV_TRY(d.pk.ensure(n * 32));
    CV_TRY(d.sig.ensure(n * 64));
    hipStream_t s = d.stream;
    auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });   // the pageable copies read the caller's arrays
    CV_TRY(hipMemcpyAsync(d.seed.p, seed + b * 32, n * 32, hipMemcpyHostToDevice, s));
    if (hi > lo) CV_TRY(hipMemcpyAsync(d.arena.p, arena + lo, hi - lo, hipMemcpyHostToDevice, s));
    CV_TRY(hipMemcpyAsync(d.off.p, off + b, n * 8, hipMemcpyHostToDevice, s));
    CV_TRY(hipMemcpyAsync(d.len.p, len + b, n * 4, hipMemcpyHostToDevice, s));
    CV_TRY(cvk_sign((uint32_t)n, d.seed.as<uint8_t>(), d.arena.as<uint8_t>() - lo, d.off.as<uint64_t>(),
                    d.len.as<uint32_t>(), d.pk.as<uint8_t>(), d.sig.as<uint8_t>(), s));
    CV_TRY(hipMemcpyAsync(pk + b * 32, d.pk.p, n * 32, hipMemcpyDeviceToHost, s));
    CV_TRY(hipMemcpyAsync(sig + b * 64, d.sig.p, n * 64, hipMemcpyDeviceToHost, s));
    CV_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    return CV_OK;
}

int cv_ed25519_sign_batch(cv_ctx *ctx, size_t n, const uint8_t *seed, const uint8_t *msg_arena,
                          const uint64_t *msg_off, const uint32_t *msg_len, uint8_t *pk_out, uint8_t *sig_out) {
    if (!ctx) return CV_E_ARGS;
    if (n == 0) return CV_OK;
    if (!seed || !msg_off || !msg_len || !pk_out || !sig_out) return CV_E_ARGS;
    const Opts o = ctx->opts();
    return dispatch(ctx, o, n, 64, [&](Device &d, size_t b, size_t e, int) {
        return sign_shard(d, b, e, seed, msg_arena, msg_off, msg_len, pk_out, sig_out);
    });
}

// ---------------------------------------------------------------- fixed-key signing (cv_signer)
// struct cv_signer is cv_host.h's: cv_api_notary.cpp signs with the record of the uniqueness set's device.

static void wipe(volatile uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; i++) p[i] = 0;
}

int cv_signer_open(cv_ctx *ctx, const uint8_t seed[32], cv_signer **out) {
    if (out) *out = nullptr;
    if (!ctx || !seed || !out) return CV_E_ARGS;
    std::unique_ptr<cv_signer> s(new (std::nothrow) cv_signer());
    if (!s) return CV_E_OOM;
    s->ctx = ctx;
    s->rec.assign(ctx->devs.size(), nullptr);
    // the seed goes up from pinned memory (a pageable copy would pass through the runtime's own staging
    // buffers), the public key comes back into it; wiped before it is freed.  Portable: every device of the
    // context copies from and to it
    uint8_t *pin = nullptr;
    int rc = hip_rc(hipSetDevice(ctx->devs[0]->ordinal));
    if (rc == CV_OK) rc = hip_rc(hipHostMalloc(reinterpret_cast<void **>(&pin), 64, hipHostMallocPortable));
    for (size_t k = 0; k < ctx->devs.size() && rc == CV_OK; k++) {
        Device &d = *ctx->devs[k];
        std::lock_guard<std::mutex> g(d.mu);
        std::memcpy(pin, seed, 32);
        auto step = [&](hipError_t e) { return rc == CV_OK ? (rc = hip_rc(e)) == CV_OK : false; };
        uint8_t *r = nullptr;
        if (!step(hipSetDevice(d.ordinal)) || !step(hipMalloc(reinterpret_cast<void **>(&r), CVK_SIGN_REC_BYTES))) break;
        s->rec[k] = r;
        step(hipMemcpyAsync(r + 96, pin, 32, hipMemcpyHostToDevice, d.stream));
        step(cvk_key_expand(reinterpret_cast<uint32_t *>(r), d.stream));
        step(hipMemcpyAsync(pin + 32, r + 64, 32, hipMemcpyDeviceToHost, d.stream));
        if (hipStreamSynchronize(d.stream) != hipSuccess && rc == CV_OK) rc = CV_E_HIP;
        if (rc == CV_OK) std::memcpy(s->pk, pin + 32, 32);
    }
    if (pin) {
        wipe(pin, 64);
        (void)hipHostFree(pin);
    }
    if (rc != CV_OK) {
        cv_signer_close(s.release());
        return rc;
    }
    *out = s.release();
    return CV_OK;
}

int cv_signer_public_key(const cv_signer *s, uint8_t pk[32]) {
    if (!s || !pk) return CV_E_ARGS;
    std::memcpy(pk, s->pk, 32);
    return CV_OK;
}

void cv_signer_close(cv_signer *s) {
    if (!s) return;
    for (size_t k = 0; k < s->rec.size(); k++) {
        if (!s->rec[k]) continue;
        Device &d = *s->ctx->devs[k];
        std::lock_guard<std::mutex> g(d.mu);
        (void)hipSetDevice(d.ordinal);
        (void)hipDeviceSynchronize();                  // signing calls still queued read the record
        (void)hipMemset(s->rec[k], 0, CVK_SIGN_REC_BYTES);
        (void)hipFree(s->rec[k]);
    }
    delete s;
}

// One shard on device d: staged like sign_shard, minus the seeds and public keys.
static int sign_keyed_shard(Device &d, const uint32_t *rec, size_t b, size_t e, const uint8_t *arena, const uint64_t *off,
                            const uint32_t *len, uint8_t *sig) {
    const size_t n = e - b;
    if (n == 0) return CV_OK;
    if (n > 0xffffffffull) return CV_E_TOO_LARGE;
    CV_TRY(hipSetDevice(d.ordinal));
    uint64_t lo = UINT64_MAX, hi = 0;
    for (size_t i = b; i < e; i++) {
        if (off[i] + len[i] < off[i]) return CV_E_ARGS;   // wraps (an unchecked call: cv_msg_extent caught the rest)
        lo = std::min<uint64_t>(lo, off[i]);
        hi = std::max<uint64_t>(hi, off[i] + len[i]);
    }
    CV_TRY(d.arena.ensure(hi - lo + 16));
    CV_TRY(d.off.ensure(n * 8));
    CV_TRY(d.len.ensure(n * 4));
    CV_TRY(d.sig.ensure(n * 64));
    hipStream_t s = d.stream;
    auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });   // the pageable copies read the caller's arrays
    if (hi > lo) CV_TRY(hipMemcpyAsync(d.arena.p, arena + lo, hi - lo, hipMemcpyHostToDevice, s));
    CV_TRY(hipMemcpyAsync(d.off.p, off + b, n * 8, hipMemcpyHostToDevice, s));
    CV_TRY(hipMemcpyAsync(d.len.p, len + b, n * 4, hipMemcpyHostToDevice, s));
    CV_TRY(cvk_sign_keyed((uint32_t)n, rec, d.arena.as<uint8_t>() - lo, d.off.as<uint64_t>(), d.len.as<uint32_t>(),
                          d.sig.as<uint8_t>(), s));
    CV_TRY(hipMemcpyAsync(sig + b * 64, d.sig.p, n * 64, hipMemcpyDeviceToHost, s));
    CV_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    return CV_OK;
}

int cv_ed25519_sign_keyed(cv_ctx *ctx, const cv_signer *s, size_t n, const uint8_t *msg_arena,
                          uint64_t msg_arena_bytes, const uint64_t *msg_off, const uint32_t *msg_len,
                          uint8_t *sig_out) {
    if (!ctx || !s || s->ctx != ctx) return CV_E_ARGS;
    if (n == 0) return CV_OK;
    if (!msg_off || !msg_len || !sig_out) return CV_E_ARGS;
    // the saturating extent: a record past the arena, or one whose off + len wraps, fails before any copy or launch
    const uint64_t extent = cv_msg_extent(n, msg_off, msg_len);
    if (extent > msg_arena_bytes || (extent && !msg_arena)) return CV_E_ARGS;
    const Opts o = ctx->opts();
    return dispatch(ctx, o, n, 64, [&](Device &d, size_t b, size_t e, int) {
        return sign_keyed_shard(d, signer_rec(s, d), b, e, msg_arena, msg_off, msg_len, sig_out);
    });
}

int cv_ed25519_sign_device(cv_ctx *ctx, int device, size_t n, const void *d_seed, const void *d_arena,
                           const void *d_off, const void *d_len, void *d_pk, void *d_sig, void *stream) {
    if (!ctx) return CV_E_ARGS;
    if (n == 0) return CV_OK;
    if (n > 0xffffffffull) return CV_E_TOO_LARGE;
    Device *d = find_dev(ctx, device);
    if (!d || !d_seed || !d_arena || !d_off || !d_len || !d_pk || !d_sig) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(d->mu);
    CV_TRY(hipSetDevice(d->ordinal));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : d->stream;
    CV_TRY(cvk_sign((uint32_t)n, static_cast<const uint8_t *>(d_seed), static_cast<const uint8_t *>(d_arena),
                    static_cast<const uint64_t *>(d_off), static_cast<const uint32_t *>(d_len),
                    static_cast<uint8_t *>(d_pk), static_cast<uint8_t *>(d_sig), s));
    return CV_OK;
}

int cv_ed25519_sign_keyed_device(cv_ctx *ctx, int device, const cv_signer *sg, size_t n, const void *d_arena,
                                 const void *d_off, const void *d_len, void *d_sig, void *stream) {
    if (!ctx || !sg || sg->ctx != ctx) return CV_E_ARGS;
    if (n == 0) return CV_OK;
    if (n > 0xffffffffull) return CV_E_TOO_LARGE;
    Device *d = find_dev(ctx, device);
    if (!d || !d_arena || !d_off || !d_len || !d_sig) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(d->mu);              // enqueue only
    CV_TRY(hipSetDevice(d->ordinal));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : d->stream;
    CV_TRY(cvk_sign_keyed((uint32_t)n, signer_rec(sg, *d), static_cast<const uint8_t *>(d_arena),
                          static_cast<const uint64_t *>(d_off), static_cast<const uint32_t *>(d_len),
                          static_cast<uint8_t *>(d_sig), s));
    return CV_OK;
}

}  // extern "C"
