// cv_api_notary.cpp — the notary's commit step of the C-ABI in one call (include/cordaverify.h): cv_notarise_batch.
// The decisions between the stages are cv_notary.h's; the set, the signer and the engine state are cv_host.h's.
//
// Everything runs on the uniqueness set's stream under the set's mutex: ONE upload of the inputs (packed in pinned
// memory), leaf hashes -> state keys -> ids, the signatures' message references and the verify (the device-resident
// verify path, which orders the shared verify workspace across streams), missing signers, the gate, the set's
// front / rounds / finish (cv_api_uniq.cpp's uniq_decide, as cv_uniq_commit_batch runs it), finalise, the signing of
// the accepted ids and their scatter, ONE read-back of the outputs (through pinned memory).  The checks of the ranges
// and the leaves, the buffer's layout, the pack list and the read-back are cv_batch.h's.
#include "cv_batch.h"

using namespace cvh;

static_assert(CV_NS_SUCCESS == CVN_SUCCESS && CV_NS_EMPTY == CVN_EMPTY && CV_NS_ID_MISMATCH == CVN_ID_MISMATCH &&
                  CV_NS_TIMESTAMP_INVALID == CVN_TIMESTAMP_INVALID && CV_NS_TX_INVALID == CVN_TX_INVALID &&
                  CV_NS_BAD_KEY == CVN_BAD_KEY && CV_NS_SIGNATURES_MISSING == CVN_SIGNATURES_MISSING &&
                  CV_NS_MALFORMED == CVN_MALFORMED && CV_NS_CONFLICT == CVN_CONFLICT && CV_VS_MISSING == CVN_VS_MISSING &&
                  CV_VS_MALFORMED == CVN_VS_MALFORMED && CV_UNIQ_CONFLICT == CVN_UNIQ_CONFLICT &&
                  CV_SIG_BAD_KEY == CVN_SIG_BAD_KEY && CVN_D_ACCEPTED > CVU_D_BAD && CVN_D_ACCEPTED < CVU_D_ROUND0,
              "cv_notary.h, cv_uniq.h and the public header agree");

extern "C" {

int cv_notarise_batch(cv_ctx *ctx, cv_uniq *u, const cv_signer *sg, int validating, size_t ntx,
                      const uint8_t *leaf_arena, uint64_t leaf_arena_bytes, const uint64_t *leaf_off,
                      const uint32_t *leaf_len, const uint32_t *tx_leaf_begin, const uint32_t *tx_input_count,
                      const uint8_t *claimed_id, const uint32_t *caller, const uint8_t *tx_pre, const uint8_t *pk,
                      const uint8_t *sig, const uint32_t *tx_sig_begin, const uint8_t *sig_pre, size_t nreq, size_t nnodes,
                      size_t nchild, const uint8_t *kind, const uint8_t *leaf_key, const int32_t *threshold,
                      const uint32_t *child_begin, const uint32_t *child, const int32_t *weight,
                      const uint32_t *req_begin, const uint32_t *tx_req_begin, const uint8_t *sig_key,
                      const uint8_t *req_allowed, uint8_t *outcome, uint8_t *ids, uint8_t *notary_sig, uint32_t *first_bad,
                      uint8_t *req_missing, uint8_t *state_conflict, uint8_t *consumed_id, uint32_t *consumed_index,
                      uint32_t *consumed_caller) {
    if (ntx == 0) return CV_OK;
    const bool val = validating != 0;
    if (!val) nreq = nnodes = nchild = 0;
    if (ntx > 0xfffffffeull || nreq > 0xfffffffeull || nnodes > 0xfffffffeull || nchild > 0xfffffffeull)
        return CV_E_TOO_LARGE;
    if (!tx_leaf_begin || !tx_input_count || !claimed_id || !caller || !outcome || !notary_sig) return CV_E_ARGS;
    if (!ranges_ok(tx_leaf_begin, ntx)) return CV_E_ARGS;
    const size_t T = ntx, L = tx_leaf_begin[T];
    if (L > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (L && (!leaf_off || !leaf_len)) return CV_E_ARGS;
    size_t S = 0;
    for (size_t t = 0; t < T; t++) {
        if (tx_input_count[t] > tx_leaf_begin[t + 1] - tx_leaf_begin[t]) return CV_E_ARGS;
        S += tx_input_count[t];
    }
    if (T > kUniqMaxStates || S > kUniqMaxStates) return CV_E_TOO_LARGE;
    if (S && (!state_conflict || !consumed_id || !consumed_index || !consumed_caller)) return CV_E_ARGS;
    size_t N = 0;
    if (val) {
        if (!tx_sig_begin || !tx_req_begin || !req_begin) return CV_E_ARGS;
        if (!ranges_ok(tx_sig_begin, T)) return CV_E_ARGS;
        N = tx_sig_begin[T];
        if (N > 0xfffffffeull) return CV_E_TOO_LARGE;
        if (N && (!pk || !sig || !sig_key)) return CV_E_ARGS;
        if (!ranges_ok(tx_req_begin, T, nreq) || !ranges_ok(req_begin, nreq, nnodes)) return CV_E_ARGS;
        if (nnodes && (!kind || !leaf_key || !threshold || !child_begin)) return CV_E_ARGS;
        if (nchild && (!child || !weight)) return CV_E_ARGS;
        if (nnodes ? (child_begin[0] != 0 || child_begin[nnodes] != nchild) : nchild != 0) return CV_E_ARGS;
    }
    // the leaves' extent: a record past the arena, or one whose off + len wraps, fails before any copy or launch
    const Extent ext = arena_extent(0, L, leaf_off, leaf_len, leaf_arena_bytes);
    const uint64_t lo = ext.lo, hi = ext.hi;
    if (!ext.ok || (hi > lo && !leaf_arena)) return CV_E_ARGS;
    if (!ctx || !u || !sg || u->ctx != ctx || sg->ctx != ctx) return CV_E_ARGS;
    const uint32_t *rec = signer_rec(sg, u->ordinal);
    if (!rec) return CV_E_ARGS;

    std::lock_guard<std::mutex> g(u->mu);
    if (u->resident + S > u->capacity) return CV_E_OOM;          // before any change and any output
    CV_TRY(hipSetDevice(u->ordinal));
    // inputs (one upload) | workspace | outputs (one read-back)
    Layout lay;
    const size_t R = nreq, W = (N + 63) / 64, bs = uniq_bslots(S);
    const size_t i_arena = lay.take(hi - lo), i_loff = lay.take(8 * L), i_llen = lay.take(4 * L);
    const size_t i_txb = lay.take(4 * (T + 1)), i_claim = lay.take(32 * T), i_cal = lay.take(4 * T), i_tpre = lay.take(T);
    const size_t i_sbeg = lay.take(4 * (T + 1)), i_sleaf = lay.take(4 * S), i_pk = lay.take(32 * N);
    const size_t i_sig = lay.take(64 * N), i_tsb = lay.take(val ? 4 * (T + 1) : 0), i_spre = lay.take(N);
    const size_t i_kind = lay.take(nnodes), i_lkey = lay.take(32 * nnodes), i_thr = lay.take(4 * nnodes);
    const size_t i_cb = lay.take(val ? 4 * (nnodes + 1) : 0);
    const size_t i_child = lay.take(4 * nchild), i_w = lay.take(4 * nchild), i_rb = lay.take(val ? 4 * (R + 1) : 0);
    const size_t i_trb = lay.take(val ? 4 * (T + 1) : 0), i_skey = lay.take(32 * N), i_allow = lay.take(R);
    const size_t in_bytes = lay.top;
    const size_t w_ldig = lay.take(32 * L), w_mst = lay.take(T), w_voff = lay.take(8 * N), w_vlen = lay.take(4 * N);
    const size_t w_bm = lay.take(8 * W), w_sst = lay.take(N), w_ck = lay.take(val ? (size_t)cvck_ws_bytes(T, nnodes) : 0);
    const size_t w_ckst = lay.take(T), w_pre = lay.take(T), w_en = lay.take(T), w_key = lay.take(32 * S);
    const size_t w_bt = lay.take(4 * bs), w_rep = lay.take(4 * S), w_res = lay.take(4 * S), w_stx = lay.take(4 * S);
    const size_t w_own = lay.take(4 * S), w_last = lay.take(4 * S), w_s0 = lay.take(4 * T), w_s1 = lay.take(4 * T);
    const size_t w_ust = lay.take(T), w_list = lay.take(4 * T), w_soff = lay.take(8 * T), w_slen = lay.take(4 * T);
    const size_t w_csig = lay.take(64 * T);
    FusedKeyed fk;                                           // CV_OPT_FUSED_KEYED: no pieces unless the call dedupes
    fk.plan(ctx->opts(), ctx->key_cap.load(), N, lay);
    const size_t o_out = lay.take(T), o_ids = lay.take(32 * T), o_fb = lay.take(4 * T), o_miss = lay.take(R);
    const size_t o_sc = lay.take(S), o_cid = lay.take(32 * S), o_cix = lay.take(4 * S), o_cc = lay.take(4 * S);
    const size_t o_nsig = lay.take(64 * T);
    const size_t out_bytes = lay.top - o_out, total = lay.top + 16;
    CV_TRY(u->nin.ensure(in_bytes + 16));
    CV_TRY(u->nout.ensure(std::max(out_bytes, fk.pinned_bytes()) + 16));
    CV_TRY(u->nws.ensure(total));

    // pack: the leaf offsets rebased to the copied part of the arena; the states' prefix sum and leaf indices
    uint8_t *h = u->nin.as<uint8_t>();
    Pack in{h};
    in.put(i_arena, leaf_arena ? leaf_arena + lo : nullptr, hi - lo);
    uint64_t *hoff = at<uint64_t>(h, i_loff);
    for (size_t i = 0; i < L; i++) hoff[i] = leaf_off[i] - lo;
    in.put(i_llen, leaf_len, 4 * L);
    in.put(i_txb, tx_leaf_begin, 4 * (T + 1));
    in.put(i_claim, claimed_id, 32 * T);
    in.put(i_cal, caller, 4 * T);
    if (tx_pre) in.put(i_tpre, tx_pre, T);
    uint32_t *hsb = at<uint32_t>(h, i_sbeg), *hsl = at<uint32_t>(h, i_sleaf);
    size_t ns = 0;
    for (size_t t = 0; t < T; t++) {
        hsb[t] = (uint32_t)ns;
        for (uint32_t j = 0; j < tx_input_count[t]; j++) hsl[ns++] = tx_leaf_begin[t] + j;
    }
    hsb[T] = (uint32_t)ns;
    if (val) {
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
        if (req_allowed) in.put(i_allow, req_allowed, R);
    }
    // the copies, from 4 MB up over the set's own host threads (CV_OPT_HOST_THREADS, as the verify pipeline packs
    // pageable inputs)
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int threads = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->opt[CV_OPT_HOST_THREADS].load(), hw));
    if (in.wants_pool(threads) && (!u->pool || u->pool->threads() != threads)) u->pool.reset(new WorkerPool(threads - 1));
    in.run(in.wants_pool(threads) ? u->pool.get() : nullptr);

    uint8_t *base = u->nws.as<uint8_t>();
    hipStream_t s = u->stream;
    auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });
    int rc = u->stat_begin();
    if (rc != CV_OK) return rc;
    CV_TRY(hipMemcpyAsync(base, h, in_bytes, hipMemcpyHostToDevice, s));
    // the key dedupe ahead of the Merkle kernels; its count and keys come back through the outputs' pinned block
    CV_TRY(fk.enqueue(base, base + i_pk, key_seed(1) | 1, u->nout.p, s, base + i_sig, base + w_voff, base + w_vlen));

    uint32_t *const d_llen = at<uint32_t>(base, i_llen), *const d_txb = at<uint32_t>(base, i_txb);
    uint32_t *const d_tsb = at<uint32_t>(base, i_tsb), *const d_ldig = at<uint32_t>(base, w_ldig);
    uint64_t *const d_loff = at<uint64_t>(base, i_loff), *const d_bm = at<uint64_t>(base, w_bm);
    CvNotary Q{};
    Q.ntx = (uint32_t)T, Q.nstates = (uint32_t)S, Q.validating = val ? 1 : 0;
    Q.mstatus = base + w_mst, Q.id = at<uint32_t>(base, o_ids), Q.claimed = at<uint32_t>(base, i_claim);
    Q.tx_pre = tx_pre ? base + i_tpre : nullptr;
    Q.tx_sig_begin = d_tsb, Q.bitmap = d_bm, Q.sig_status = base + w_sst;
    Q.sig_pre = val && sig_pre ? base + i_spre : nullptr, Q.ck_status = base + w_ckst;
    Q.pre = base + w_pre, Q.enable = base + w_en, Q.first_bad = at<uint32_t>(base, o_fb);
    Q.leaf_digest = d_ldig, Q.state_leaf = at<uint32_t>(base, i_sleaf), Q.key = at<uint32_t>(base, w_key);
    Q.uniq_status = base + w_ust, Q.outcome = base + o_out;
    Q.list = at<uint32_t>(base, w_list), Q.sign_off = at<uint64_t>(base, w_soff), Q.sign_len = at<uint32_t>(base, w_slen);

    // leaf hashes, the state keys out of them, then the trees (which fold the digests in place)
    CV_TRY(cvk_merkle(0, (uint32_t)L, 0, base + i_arena, d_loff, d_llen, d_txb, d_ldig, nullptr, nullptr, s));
    CV_TRY(cvk_notary_gather(&Q, s));
    CV_TRY(cvk_merkle((uint32_t)T, 0, 0, base + i_arena, d_loff, d_llen, d_txb, d_ldig, base + o_ids, base + w_mst, s));
    if (val) {
        if (N) {
            CV_TRY(cvk_tx_sig_refs((uint32_t)N, 0, (uint32_t)T, 0, d_tsb, at<uint64_t>(base, w_voff),
                                   at<uint32_t>(base, w_vlen), s));
            size_t nkeys = 0;
            rc = fk.decide(u->nout.p, &nkeys);
            if (rc != CV_OK) return rc;
            if (fk.hot) {
                Device &d = *find_dev(ctx, u->ordinal);
                std::lock_guard<std::mutex> gd(d.mu);
                rc = fk.verify_hot(ctx, d, u->nout.p, base + o_ids, d_bm, base + w_sst, s);
            } else if (nkeys) {
                // the key pool is the device's: its lock inside the set's, as the unkeyed call below takes it
                Device &d = *find_dev(ctx, u->ordinal);
                std::lock_guard<std::mutex> gd(d.mu);
                rc = verify_keyed_locked(ctx, d, N, nkeys, fk.host_keys(u->nout.p), base + fk.keys,
                                         at<uint32_t>(base, fk.kidx), base + i_sig, base + o_ids, at<uint64_t>(base, w_voff),
                                         at<uint32_t>(base, w_vlen), d_bm, base + w_sst, s, nullptr);
            } else
                rc = cv_ed25519_verify_device(ctx, u->ordinal, N, base + i_pk, base + i_sig, base + o_ids, base + w_voff,
                                              base + w_vlen, base + w_bm, base + w_sst, s);
            if (rc != CV_OK) return rc;
        }
        const CvCk a = ck_args(base, {T, R, nnodes, nchild, N},
                               {i_kind, i_lkey, i_thr, i_cb, i_child, i_w, i_rb, i_trb, i_skey, i_tsb, i_allow, w_bm, w_ck,
                                o_miss, w_ckst},
                               req_allowed != nullptr, N != 0, 0);
        CV_TRY(cvk_ck(&a, s));
    }
    CV_TRY(cvk_notary_gate(&Q, s));
    // records of states without a conflict and signatures of transactions that are not committed: zero
    CV_TRY(hipMemsetAsync(base + o_cid, 0, lay.top - o_cid, s));
    CvUniqBatch B{};
    B.ntx = (uint32_t)T, B.nstates = (uint32_t)S;
    B.key = Q.key, B.begin = at<uint32_t>(base, i_sbeg), B.id = Q.id, B.caller = at<uint32_t>(base, i_cal);
    B.enable = base + w_en, B.btab = at<uint32_t>(base, w_bt), B.bmask = (uint32_t)(bs - 1);
    B.rep = at<uint32_t>(base, w_rep), B.res = at<uint32_t>(base, w_res), B.state_tx = at<uint32_t>(base, w_stx);
    B.owner = at<uint32_t>(base, w_own), B.last = at<uint32_t>(base, w_last);
    B.tx_status = base + w_ust, B.state_conflict = base + o_sc;
    B.cons_id = at<uint32_t>(base, o_cid), B.cons_index = at<uint32_t>(base, o_cix);
    B.cons_caller = at<uint32_t>(base, o_cc);
    B.dstat = u->dstat.as<uint32_t>();
    uint64_t rounds = 0;
    rc = uniq_decide(u, B, at<uint32_t>(base, w_s0), at<uint32_t>(base, w_s1), &rounds);
    if (rc != CV_OK) return rc;
    CV_TRY(cvk_notary_final(&Q, B.dstat + CVN_D_ACCEPTED, s));
    rc = uniq_stat_end(u);                                       // synchronises: the accepted count is on the host
    u->resident += u->hstat[CVU_D_INSERTED];
    u->last_rounds = rounds;
    u->last_tail = u->hstat[CVU_D_TAIL];
    if (rc != CV_OK) {
        drain.armed = false;
        return rc;
    }
    const uint32_t count = u->hstat[CVN_D_ACCEPTED];
    if (count > T) return CV_E_HIP;
    // the signing kernel runs for the accepted transactions alone, into a compact array; the scatter places them
    CV_TRY(cvk_sign_keyed(count, rec, base + o_ids, Q.sign_off, Q.sign_len, base + w_csig, s));
    CV_TRY(cvk_notary_scatter(count, Q.list, base + w_csig, base + o_nsig, s));
    const Unpack out{u->nout.as<uint8_t>(), o_out};
    CV_TRY(hipMemcpyAsync(u->nout.p, base + o_out, out_bytes, hipMemcpyDeviceToHost, s));
    CV_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    out.get(outcome, o_out, T);
    out.get(ids, o_ids, 32 * T);
    out.get(first_bad, o_fb, 4 * T);
    out.get(req_missing, o_miss, R);
    out.get(state_conflict, o_sc, S);
    out.get(consumed_id, o_cid, 32 * S);
    out.get(consumed_index, o_cix, 4 * S);
    out.get(consumed_caller, o_cc, 4 * S);
    out.get(notary_sig, o_nsig, 64 * T);
    return CV_OK;
}

}  // extern "C"
