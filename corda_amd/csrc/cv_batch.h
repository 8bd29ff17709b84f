// cv_batch.h — what the one-shot batch calls of the C-ABI library share (cv_api_{sign,pmt,uniq,ck,notary,tearoff}.cpp):
// the checks of their range and record arrays, the layout of the one device buffer a call carves up (inputs |
// workspace | outputs), the pack list of a call that uploads once from pinned memory and its read-back, the signer's
// record for a device, routing to one device, and CvCk from a base and its offsets.  Host only: built on cv_host.h,
// included by no .hip file and no kernel-side header.  Everything here is defined once, inline, in namespace cvh.
#pragma once
#include "cv_host.h"

namespace cvh {

// ---------------------------------------------------------------- checks
// n ranges in begin[0 .. n]: begin[0] == 0 and monotone (the last entry is the count); with total, begin[n] == total
inline bool ranges_ok(const uint32_t *begin, size_t n) {
    if (begin[0] != 0) return false;
    for (size_t i = 0; i < n; i++)
        if (begin[i + 1] < begin[i]) return false;
    return true;
}
inline bool ranges_ok(const uint32_t *begin, size_t n, size_t total) { return begin[n] == total && ranges_ok(begin, n); }

// The part [lo, hi) of an arena that records [b, e) reach (0, 0 for none) and whether all of them lie inside
// arena_bytes.  arena_span saturates the end of a record whose off + len wraps, so the one comparison rejects that
// record too (also against an arena "without end": nothing ends at 2^64 - 1).
struct Extent {
    uint64_t lo, hi;
    bool ok;
};
inline Extent arena_extent(size_t b, size_t e, const uint64_t *off, const uint32_t *len, uint64_t arena_bytes) {
    const Span sp = arena_span(b, e, off, len, nullptr);
    return {sp.lo, sp.hi, sp.hi <= std::min(arena_bytes, UINT64_MAX - 1)};
}

// ---------------------------------------------------------------- layout
// Offsets of the pieces of one buffer, in the order they are taken, each 16-byte aligned; top: the bytes taken so far.
struct Layout {
    size_t top = 0;
    size_t take(size_t bytes) {
        const size_t at = top;
        top += al16(bytes);
        return at;
    }
};
template <class T> inline T *at(uint8_t *base, size_t off) { return reinterpret_cast<T *>(base + off); }

// ---------------------------------------------------------------- pack and unpack (pinned memory)
// The copies of a call that packs its inputs into the pinned block h for ONE upload: put() lists a caller's array
// for its offset (nothing for zero bytes, whatever src is), run() copies — one after another for a notary-sized
// batch, cut into 256 KB tasks over host threads from 4 MB up (par_copy).  wants_pool() says whether run() needs
// them, so a caller creates its pool for the first large batch only.
struct Pack {
    static constexpr size_t kParMin = (size_t)4 << 20;
    uint8_t *h;
    std::vector<CopyJob> jobs;
    size_t bytes = 0;
    void put(size_t off, const void *src, size_t n) {
        if (!n) return;
        jobs.push_back({h + off, src, n});
        bytes += n;
    }
    bool wants_pool(int threads) const { return bytes >= kParMin && threads > 1; }
    void run(WorkerPool *workers) const { par_copy(jobs, workers, kParMin); }
};
// The read-back of such a call: h holds the device buffer from offset `first` on; get() copies the piece at device
// offset off to the caller (nothing for a null dst or zero bytes).
struct Unpack {
    const uint8_t *h;
    size_t first;
    void get(void *dst, size_t off, size_t n) const {
        if (dst && n) std::memcpy(dst, h + (off - first), n);
    }
};

// ---------------------------------------------------------------- signer, routing
// the signer's record for a device of its context (by reference, or by ordinal), or null
inline const uint32_t *signer_rec(const cv_signer *sg, const Device &d) {
    const size_t k = dev_index(sg->ctx, d);
    return k < sg->rec.size() ? static_cast<const uint32_t *>(sg->rec[k]) : nullptr;
}
inline const uint32_t *signer_rec(const cv_signer *sg, int ordinal) {
    const Device *d = find_dev(sg->ctx, ordinal);
    return d ? signer_rec(sg, *d) : nullptr;
}

// dispatch for a small batch: the whole of it on one device, the least loaded
template <class F> inline int dispatch_one(cv_ctx *ctx, size_t n, F fn) {
    Opts o = ctx->opts();
    o.shard_min = o.spread_min = SIZE_MAX;
    return dispatch(ctx, o, n, 1, fn);
}

// ---------------------------------------------------------------- the keyed route of the fused calls
// CV_OPT_FUSED_KEYED for cv_notarise_batch and cv_resolve_batch, in the order a call uses it:
//   plan     whether the call dedupes its n signatures' keys at all — mode 2, or mode 1 with n above the tri-chain size
//            (below it the rule keeps the unkeyed path whatever the keys) — the most key rows it would read back
//            (floor(n / 8) under mode 1, n under mode 2, the pool's capacity under both) and its pieces of the call's
//            device buffer: head (the count) | keys, read back as one piece, | key_index | the dedupe's workspace
//   enqueue  right after the upload: the dedupe (it needs the keys alone, so it runs ahead of the Merkle kernels), the
//            copy of head and rows into the call's pinned block, an event behind it
//   decide   before the verify: waits for the event — the one synchronisation the route adds; the kernels enqueued
//            since run meanwhile — and gives the distinct keys when the call takes the keyed path, 0 when it stays
//            unkeyed (more keys than rows), CV_E_HIP after a probe error
// Modes 3 and 4 are the hot-key route (cv_hotkeys.h) in the same three places: plan takes the route's
// workspace as one piece (mode 3: more than the tri-chain size, hot_min 8; mode 4: any batch, hot_min 2), enqueue runs
// hotkeys_front (the read-back is head | the hot key rows only), decide waits for it and leaves the keyed count 0, and
// the call hands its verify to verify_hot — verify_hotkeys_locked — in place of the two branches, behind
// cvk_tx_sig_refs, whose message references the record gather copies.
struct FusedKeyed {
    bool want = false, hot = false;
    size_t n = 0, rows = 0, head = 0, keys = 0, kidx = 0, ws = 0;
    CvdLayout L{};
    CvhLayout HL{};
    CvHot H{};
    uint32_t hot_min = 0, hot_cap = 0;
    hipEvent_t ev = nullptr;
    ~FusedKeyed() {
        if (ev) (void)hipEventDestroy(ev);
    }
    void plan(const Opts &o, uint32_t key_cap, size_t nsig, Layout &lay) {
        n = nsig;
        if (o.fused_keyed >= 3) {
            hot_min = o.fused_keyed == 4 ? 2 : CVH_HOT_MIN_DEFAULT, hot_cap = key_cap;
            rows = (size_t)cvh_rows(n, hot_min, hot_cap);
            want = hot = rows != 0 && (o.fused_keyed == 4 || n > o.plan.tri_max);
            if (!want) return;
            HL = cvh_layout(n);
            ws = lay.take((size_t)HL.bytes);
            return;
        }
        rows = std::min<size_t>(o.fused_keyed == 2 ? n : n / 8, key_cap);
        want = rows != 0 && (o.fused_keyed == 2 || (o.fused_keyed == 1 && n > o.plan.tri_max));
        if (!want) return;
        L = cvd_layout(n);
        head = lay.take(16), keys = lay.take(32 * n), kidx = lay.take(4 * n), ws = lay.take((size_t)L.bytes);
    }
    size_t pinned_bytes() const { return want ? 16 + 32 * rows : 0; }
    // d_sig, d_off, d_len: the records the hot-key route gathers (d_off / d_len may be written later on the stream)
    hipError_t enqueue(uint8_t *base, const uint8_t *d_pk, uint64_t seed, void *pin, hipStream_t s,
                       const void *d_sig = nullptr, const void *d_off = nullptr, const void *d_len = nullptr) {
        if (!want) return hipSuccess;
        if (hot) {
            H = cvh_args(n, hot_min, hot_cap, d_pk, d_sig, d_off, d_len, base + ws, HL);
            hipError_t e = hotkeys_front(H, HL, base + ws, seed, rows, pin, s);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(ev, s);
            return e;
        }
        const CvDedupe D = cvd_args(n, d_pk, base + keys, base + kidx, base + head, base + ws, seed, L);
        uint32_t *sums[CVD_LEVELS];
        for (int k = 0; k < CVD_LEVELS; k++) sums[k] = at<uint32_t>(base, ws + (size_t)L.sum[k]);
        hipError_t e = cvk_dedupe(&D, sums, s);
        if (e == hipSuccess) e = hipMemcpyAsync(pin, base + head, pinned_bytes(), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(ev, s);
        return e;
    }
    int decide(const void *pin, size_t *nkeys) const {
        *nkeys = 0;
        if (!want) return CV_OK;
        CV_TRY(hipEventSynchronize(ev));
        if (hot) return CV_OK;
        const uint32_t nk = *static_cast<const uint32_t *>(pin);
        if (nk == 0 || nk > n) return CV_E_HIP;
        if (nk <= rows) *nkeys = nk;
        return CV_OK;
    }
    // the call's verify under modes 3 and 4, after decide; the caller holds d.mu
    int verify_hot(cv_ctx *ctx, Device &d, const void *pin, const uint8_t *arena, uint64_t *bitmap, uint8_t *status,
                   hipStream_t s) const {
        return verify_hotkeys_locked(ctx, d, H, rows, pin, arena, bitmap, status, s, nullptr);
    }
    const uint8_t *host_keys(const void *pin) const { return static_cast<const uint8_t *>(pin) + 16; }
};

// ---------------------------------------------------------------- missing signers
// CvCk over one buffer: the counts and the offsets of its arrays, in CvCk's order (ws: cvck_ws_bytes of workspace).
struct CkCounts {
    size_t ntx, nreq, nnodes, nchild, nsig;
};
struct CkAt {
    size_t kind, leaf_key, threshold, child_begin, child, weight, req_begin, tx_req_begin, sig_key, tx_sig_begin;
    size_t req_allowed, bitmap, ws, req_missing, tx_status;
};
inline CvCk ck_args(uint8_t *base, const CkCounts &n, const CkAt &o, bool allowed, bool bitmap, uint32_t wide_min) {
    CvCk a{};
    a.ntx = (uint32_t)n.ntx, a.nreq = (uint32_t)n.nreq, a.nnodes = (uint32_t)n.nnodes, a.nchild = (uint32_t)n.nchild;
    a.nsig = (uint32_t)n.nsig;
    a.kind = base + o.kind, a.leaf_key = base + o.leaf_key, a.threshold = at<int32_t>(base, o.threshold);
    a.child_begin = at<uint32_t>(base, o.child_begin), a.child = at<uint32_t>(base, o.child);
    a.weight = at<int32_t>(base, o.weight), a.req_begin = at<uint32_t>(base, o.req_begin);
    a.tx_req_begin = at<uint32_t>(base, o.tx_req_begin), a.sig_key = base + o.sig_key;
    a.tx_sig_begin = at<uint32_t>(base, o.tx_sig_begin);
    a.req_allowed = allowed ? base + o.req_allowed : nullptr;
    a.bitmap = bitmap ? at<uint64_t>(base, o.bitmap) : nullptr;
    a.wide_min = wide_min;
    a.count = at<uint32_t>(base, o.ws), a.list = at<uint32_t>(base, o.ws + CVCK_WS_LIST);
    a.flag = base + o.ws + cvck_ws_flag_off(n.ntx);
    a.req_missing = base + o.req_missing, a.tx_status = base + o.tx_status;
    return a;
}

}  // namespace cvh
