// cv_api_resolve.cpp — ResolveTransactionsFlow.call over a downloaded batch of the C-ABI in one call
// (include/cordaverify.h): cv_resolve_batch.  The join, the gate, the order and the walk are cv_resolve.h's; the
// engine state is cv_host.h's.
//
// One device, the least loaded, everything in d.pmt on d.stream: ONE upload of the inputs (packed in pinned memory),
// leaf hashes -> ids, the join table's insert and probe, the signatures' message references and the verify (the
// device-resident verify path on the shared workspace), missing signers, the gate, ONE read-back of the outputs and
// the call's counters (through pinned memory); then topologicalSort and the walk on the host (cvr_finish).  The checks
// of the ranges and the leaves, the buffer's layout, the pack list and the read-back are cv_batch.h's.
#include "cv_batch.h"

using namespace cvh;

static_assert(CV_RS_OK == CVR_OK && CV_RS_EMPTY == CVR_EMPTY && CV_RS_ID_MISMATCH == CVR_ID_MISMATCH &&
                  CV_RS_TX_INVALID == CVR_TX_INVALID && CV_RS_BAD_KEY == CVR_BAD_KEY &&
                  CV_RS_SIGNATURES_MISSING == CVR_SIGNATURES_MISSING && CV_RS_MALFORMED == CVR_MALFORMED &&
                  CV_RS_BAD_INPUT == CVR_BAD_INPUT && CV_RS_UNRESOLVED == CVR_UNRESOLVED && CV_RS_EMPTY == CV_NS_EMPTY &&
                  CV_RS_ID_MISMATCH == CV_NS_ID_MISMATCH && CV_RS_TX_INVALID == CV_NS_TX_INVALID &&
                  CV_RS_BAD_KEY == CV_NS_BAD_KEY && CV_RS_SIGNATURES_MISSING == CV_NS_SIGNATURES_MISSING &&
                  CV_RS_MALFORMED == CV_NS_MALFORMED && CV_RG_OK == CVR_GS_OK && CV_RG_BAD_ID == CVR_GS_BAD_ID &&
                  CV_RG_DUPLICATE_ID == CVR_GS_DUPLICATE_ID && CV_RG_STATUS == CVR_G_STATUS && CV_RG_WHICH == CVR_G_WHICH &&
                  CV_RG_N_PASS == CVR_G_N_PASS && CV_RG_STOP_CLASS == CVR_G_STOP_CLASS && CV_RG_STOP_TX == CVR_G_STOP_TX &&
                  CV_RG_STOP_INPUT == CVR_G_STOP_INPUT && CV_RG_EXTERNAL == CVR_G_EXTERNAL &&
                  CV_RG_MAXPROBE == CVR_G_MAXPROBE && CV_RG_WRAPS == CVR_G_WRAPS && CV_RG_WORDS == CVR_G_WORDS &&
                  CV_VS_MISSING == CVN_VS_MISSING && CV_VS_MALFORMED == CVN_VS_MALFORMED && CV_SIG_BAD_KEY == CVN_SIG_BAD_KEY,
              "cv_resolve.h, cv_notary.h and the public header agree");

namespace {

constexpr size_t kResolveMax = (size_t)1 << 30;   // transactions, inputs: the table's slot count stays within 2^31

// CV_OPT_TIMELINE: events between the stages of one call (created for the call, destroyed with it)
struct StageClock {
    static constexpr int kMarks = 8;
    hipEvent_t ev[kMarks] = {};
    bool on = false;
    hipError_t start(bool want) {
        on = want;
        for (int k = 0; on && k < kMarks; k++) {
            const hipError_t e = hipEventCreate(&ev[k]);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    hipError_t mark(int k, hipStream_t s) { return on ? hipEventRecord(ev[k], s) : hipSuccess; }
    ~StageClock() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace

extern "C" {

int cv_resolve_batch(cv_ctx *ctx, size_t ntx, const uint8_t *leaf_arena, uint64_t leaf_arena_bytes,
                     const uint64_t *leaf_off, const uint32_t *leaf_len, const uint32_t *tx_leaf_begin,
                     const uint8_t *claimed_id, const uint8_t *pk, const uint8_t *sig, const uint32_t *tx_sig_begin,
                     const uint8_t *sig_pre, size_t nreq, size_t nnodes, size_t nchild, const uint8_t *kind,
                     const uint8_t *leaf_key, const int32_t *threshold, const uint32_t *child_begin, const uint32_t *child,
                     const int32_t *weight, const uint32_t *req_begin, const uint32_t *tx_req_begin, const uint8_t *sig_key,
                     size_t ninputs, const uint32_t *tx_input_begin, const uint8_t *input_txhash,
                     const uint32_t *input_index, const uint32_t *tx_output_count, uint64_t seed, uint8_t *outcome,
                     uint32_t *first_bad, uint8_t *req_missing, uint32_t *bad_input, uint32_t *input_dep,
                     uint8_t *input_status, uint32_t *order, uint32_t *graph, uint8_t *ids) {
    if (ntx == 0) return CV_OK;
    if (ntx > 0xfffffffeull || nreq > 0xfffffffeull || nnodes > 0xfffffffeull || nchild > 0xfffffffeull ||
        ninputs > 0xfffffffeull)
        return CV_E_TOO_LARGE;
    if (ntx > kResolveMax || ninputs > kResolveMax) return CV_E_TOO_LARGE;
    if (!tx_leaf_begin || !claimed_id || !tx_sig_begin || !tx_req_begin || !req_begin || !tx_input_begin ||
        !tx_output_count || !outcome || !bad_input || !order || !graph)
        return CV_E_ARGS;
    if (!ranges_ok(tx_leaf_begin, ntx) || !ranges_ok(tx_sig_begin, ntx)) return CV_E_ARGS;
    const size_t T = ntx, L = tx_leaf_begin[T], N = tx_sig_begin[T], R = nreq, I = ninputs;
    if (L > 0xfffffffeull || N > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (L && (!leaf_off || !leaf_len)) return CV_E_ARGS;
    if (N && (!pk || !sig || !sig_key)) return CV_E_ARGS;
    if (!ranges_ok(tx_req_begin, T, R) || !ranges_ok(req_begin, R, nnodes) || !ranges_ok(tx_input_begin, T, I))
        return CV_E_ARGS;
    if (nnodes && (!kind || !leaf_key || !threshold || !child_begin)) return CV_E_ARGS;
    if (nchild && (!child || !weight)) return CV_E_ARGS;
    if (nnodes ? (child_begin[0] != 0 || child_begin[nnodes] != nchild) : nchild != 0) return CV_E_ARGS;
    if (I && (!input_txhash || !input_index || !input_dep || !input_status)) return CV_E_ARGS;
    // the leaves' extent: a record past the arena, or one whose off + len wraps, fails before any copy or launch
    const Extent ext = arena_extent(0, L, leaf_off, leaf_len, leaf_arena_bytes);
    const uint64_t lo = ext.lo, hi = ext.hi;
    if (!ext.ok || (hi > lo && !leaf_arena)) return CV_E_ARGS;
    if (!ctx) return CV_E_ARGS;
    if (seed == 0) {
        std::random_device rd;
        seed = (key_seed(0) ^ (((uint64_t)rd() << 32) | rd())) | 1;
    }
    const Opts opts = ctx->opts();
    const bool timed = opts.timeline != 0;

    return dispatch_one(ctx, T, [&](Device &d, size_t, size_t, int threads) {
        CV_TRY(hipSetDevice(d.ordinal));
        // inputs (one upload) | workspace, the join table last | counters and outputs (one read-back)
        Layout lay;
        const size_t W = (N + 63) / 64, slots = cvr_slots(T);
        const size_t i_arena = lay.take(hi - lo), i_loff = lay.take(8 * L), i_llen = lay.take(4 * L);
        const size_t i_txb = lay.take(4 * (T + 1)), i_claim = lay.take(32 * T), i_pk = lay.take(32 * N);
        const size_t i_sig = lay.take(64 * N), i_tsb = lay.take(4 * (T + 1)), i_spre = lay.take(N);
        const size_t i_kind = lay.take(nnodes), i_lkey = lay.take(32 * nnodes), i_thr = lay.take(4 * nnodes);
        const size_t i_cb = lay.take(4 * (nnodes + 1)), i_child = lay.take(4 * nchild), i_w = lay.take(4 * nchild);
        const size_t i_rb = lay.take(4 * (R + 1)), i_trb = lay.take(4 * (T + 1)), i_skey = lay.take(32 * N);
        const size_t i_tib = lay.take(4 * (T + 1)), i_hash = lay.take(32 * I), i_idx = lay.take(4 * I);
        const size_t i_cnt = lay.take(4 * T), in_bytes = lay.top;
        const size_t w_ldig = lay.take(32 * L), w_mst = lay.take(T), w_voff = lay.take(8 * N), w_vlen = lay.take(4 * N);
        const size_t w_bm = lay.take(8 * W), w_sst = lay.take(N), w_ck = lay.take((size_t)cvck_ws_bytes(T, nnodes));
        FusedKeyed fk;                                       // CV_OPT_FUSED_KEYED: no pieces unless the call dedupes
        fk.plan(opts, ctx->key_cap.load(), N, lay);
        const size_t w_ckst = lay.take(T), w_tab = lay.take(4 * slots);
        const size_t o_stat = lay.take(4 * CVR_D_WORDS), o_out = lay.take(T), o_fb = lay.take(4 * T), o_miss = lay.take(R);
        const size_t o_bin = lay.take(4 * T), o_dep = lay.take(4 * I), o_ist = lay.take(I), o_ids = lay.take(32 * T);
        const size_t out_bytes = lay.top - o_stat, total = lay.top + 16;
        static_assert(CVR_D_ERROR == 4 && CVR_D_WORDS == 8, "the counters' two halves are cleared by one memset each");
        CV_TRY(d.ts_in.ensure(in_bytes + 16));
        CV_TRY(d.ts_out.ensure(std::max(out_bytes, fk.pinned_bytes()) + 16));
        CV_TRY(d.pmt.ensure(total));

        // pack: the leaf offsets rebased to the copied part of the arena
        uint8_t *h = d.ts_in.as<uint8_t>();
        Pack in{h};
        in.put(i_arena, leaf_arena ? leaf_arena + lo : nullptr, hi - lo);
        uint64_t *hoff = at<uint64_t>(h, i_loff);
        for (size_t i = 0; i < L; i++) hoff[i] = leaf_off[i] - lo;
        in.put(i_llen, leaf_len, 4 * L);
        in.put(i_txb, tx_leaf_begin, 4 * (T + 1));
        in.put(i_claim, claimed_id, 32 * T);
        in.put(i_pk, pk, 32 * N);
        in.put(i_sig, sig, 64 * N);
        in.put(i_tsb, tx_sig_begin, 4 * (T + 1));
        if (sig_pre) in.put(i_spre, sig_pre, N);
        in.put(i_kind, kind, nnodes);
        in.put(i_lkey, leaf_key, 32 * nnodes);
        in.put(i_thr, threshold, 4 * nnodes);
        if (nnodes) in.put(i_cb, child_begin, 4 * (nnodes + 1));
        in.put(i_child, child, 4 * nchild);
        in.put(i_w, weight, 4 * nchild);
        in.put(i_rb, req_begin, 4 * (R + 1));
        in.put(i_trb, tx_req_begin, 4 * (T + 1));
        in.put(i_skey, sig_key, 32 * N);
        in.put(i_tib, tx_input_begin, 4 * (T + 1));
        in.put(i_hash, input_txhash, 32 * I);
        in.put(i_idx, input_index, 4 * I);
        in.put(i_cnt, tx_output_count, 4 * T);
        in.run(in.wants_pool(threads) ? &d.workers(threads) : nullptr);

        uint8_t *base = d.pmt.as<uint8_t>();
        hipStream_t s = d.stream;
        StageClock clk;
        CV_TRY(clk.start(timed));
        auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });
        CV_TRY(clk.mark(0, s));
        CV_TRY(hipMemcpyAsync(base, h, in_bytes, hipMemcpyHostToDevice, s));
        CV_TRY(clk.mark(1, s));
        // the key dedupe ahead of the Merkle kernels; its count and keys come back through the outputs' pinned block
        CV_TRY(fk.enqueue(base, base + i_pk, seed, d.ts_out.p, s, base + i_sig, base + w_voff, base + w_vlen));

        uint32_t *const d_llen = at<uint32_t>(base, i_llen), *const d_txb = at<uint32_t>(base, i_txb);
        uint32_t *const d_tsb = at<uint32_t>(base, i_tsb), *const d_ldig = at<uint32_t>(base, w_ldig);
        CvResolve Q{};
        Q.ntx = (uint32_t)T, Q.ninputs = (uint32_t)I;
        Q.claimed = at<uint32_t>(base, i_claim), Q.tab = at<uint32_t>(base, w_tab), Q.mask = (uint32_t)(slots - 1);
        Q.seed = seed;
        Q.tx_input_begin = at<uint32_t>(base, i_tib), Q.input_txhash = at<uint32_t>(base, i_hash);
        Q.input_index = at<uint32_t>(base, i_idx), Q.tx_output_count = at<uint32_t>(base, i_cnt);
        Q.input_dep = at<uint32_t>(base, o_dep), Q.input_status = base + o_ist;
        Q.mstatus = base + w_mst, Q.id = at<uint32_t>(base, o_ids), Q.tx_sig_begin = d_tsb;
        Q.bitmap = at<uint64_t>(base, w_bm), Q.sig_status = base + w_sst, Q.sig_pre = sig_pre ? base + i_spre : nullptr;
        Q.ck_status = base + w_ckst, Q.outcome = base + o_out, Q.first_bad = at<uint32_t>(base, o_fb);
        Q.bad_input = at<uint32_t>(base, o_bin), Q.dstat = at<uint32_t>(base, o_stat);

        CV_TRY(cvk_merkle((uint32_t)T, (uint32_t)L, 0, base + i_arena, at<uint64_t>(base, i_loff), d_llen, d_txb, d_ldig,
                          base + o_ids, base + w_mst, s));
        CV_TRY(clk.mark(2, s));
        // the table empty and the atomicMin counters at their identity (they lie behind the table), the others zero
        CV_TRY(hipMemsetAsync(base + w_tab, 0xff, o_stat + 4 * CVR_D_ERROR - w_tab, s));
        CV_TRY(hipMemsetAsync(base + o_stat + 4 * CVR_D_ERROR, 0, 4 * (CVR_D_WORDS - CVR_D_ERROR), s));
        CV_TRY(cvk_resolve_join(&Q, s));
        CV_TRY(clk.mark(3, s));
        if (N) {
            CV_TRY(cvk_tx_sig_refs((uint32_t)N, 0, (uint32_t)T, 0, d_tsb, at<uint64_t>(base, w_voff),
                                   at<uint32_t>(base, w_vlen), s));
            size_t nkeys = 0;
            int rc = fk.decide(d.ts_out.p, &nkeys);
            if (rc != CV_OK) return rc;
            if (fk.hot) {
                rc = fk.verify_hot(ctx, d, d.ts_out.p, base + o_ids, at<uint64_t>(base, w_bm), base + w_sst, s);
                if (rc != CV_OK) return rc;
            } else if (nkeys) {
                rc = verify_keyed_locked(ctx, d, N, nkeys, fk.host_keys(d.ts_out.p), base + fk.keys,
                                         at<uint32_t>(base, fk.kidx), base + i_sig, base + o_ids, at<uint64_t>(base, w_voff),
                                         at<uint32_t>(base, w_vlen), at<uint64_t>(base, w_bm), base + w_sst, s, nullptr);
                if (rc != CV_OK) return rc;
            } else
                CV_TRY(verify_device_locked(ctx, d, N, base + i_pk, base + i_sig, base + o_ids, at<uint64_t>(base, w_voff),
                                            at<uint32_t>(base, w_vlen), at<uint64_t>(base, w_bm), base + w_sst, s));
        }
        CV_TRY(clk.mark(4, s));
        const CvCk a = ck_args(base, {T, R, nnodes, nchild, N},
                               {i_kind, i_lkey, i_thr, i_cb, i_child, i_w, i_rb, i_trb, i_skey, i_tsb, 0, w_bm, w_ck, o_miss,
                                w_ckst},
                               false, N != 0, 0);
        CV_TRY(cvk_ck(&a, s));
        CV_TRY(clk.mark(5, s));
        CV_TRY(cvk_resolve_gate(&Q, s));
        CV_TRY(clk.mark(6, s));
        uint8_t *ho = d.ts_out.as<uint8_t>();
        CV_TRY(hipMemcpyAsync(ho, base + o_stat, out_bytes, hipMemcpyDeviceToHost, s));
        CV_TRY(clk.mark(7, s));
        CV_TRY(hipStreamSynchronize(s));
        drain.armed = false;

        // order and the walk from the pinned copy, then the outputs to the caller
        const double t0 = timed ? now_s() : 0;
        const Unpack res{ho, o_stat};
        const uint32_t *h_dep = at<uint32_t>(ho, o_dep - o_stat);
        std::vector<uint32_t> ord(T);
        uint32_t g[CVR_G_WORDS];
        if (!cvr_finish((uint32_t)T, tx_input_begin, h_dep, ho + (o_ist - o_stat), ho + (o_out - o_stat),
                        at<uint32_t>(ho, o_bin - o_stat), at<uint32_t>(ho, 0), ord.data(), g))
            return (int)CV_E_HIP;
        res.get(outcome, o_out, T);
        res.get(first_bad, o_fb, 4 * T);
        res.get(req_missing, o_miss, R);
        res.get(bad_input, o_bin, 4 * T);
        res.get(input_dep, o_dep, 4 * I);
        res.get(input_status, o_ist, I);
        res.get(ids, o_ids, 32 * T);
        std::memcpy(order, ord.data(), 4 * T);
        std::memcpy(graph, g, sizeof g);
        if (timed) {
            double v[kRsVals] = {};
            for (int k = 0; k < 7; k++) {
                float ms = 0.f;
                CV_TRY(hipEventElapsedTime(&ms, clk.ev[k], clk.ev[k + 1]));
                v[k] = ms;
            }
            v[7] = (now_s() - t0) * 1e3;
            std::lock_guard<std::mutex> gs(ctx->st_mu);
            for (int k = 0; k < kRsVals; k++) ctx->stats.rs[k] += v[k];
            ctx->stats.rs[kRsVals] += 1;
        }
        return (int)CV_OK;
    });
}

}  // extern "C"
