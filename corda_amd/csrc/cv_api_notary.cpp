// cv_api_notary.cpp — the notary's commit step of the C-ABI in one call (include/cordaverify.h): cv_notarise_batch.
// The decisions between the stages are cv_notary.h's; the set, the signer and the engine state are cv_host.h's.
//
// Everything runs on the uniqueness set's stream under the set's mutex: ONE upload of the inputs (packed in pinned
// memory), leaf hashes -> state keys -> ids, the signatures' message references and the verify (the device-resident
// verify path, which orders the shared verify workspace across streams), missing signers, the gate, the set's
// front / rounds / finish (cv_api_uniq.cpp's uniq_decide, as cv_uniq_commit_batch runs it), finalise, the signing of
// the accepted ids and their scatter, ONE read-back of the outputs (through pinned memory).
#include "cv_host.h"

using namespace cvh;

static_assert(CV_NS_SUCCESS == CVN_SUCCESS && CV_NS_EMPTY == CVN_EMPTY && CV_NS_ID_MISMATCH == CVN_ID_MISMATCH &&
                  CV_NS_TIMESTAMP_INVALID == CVN_TIMESTAMP_INVALID && CV_NS_TX_INVALID == CVN_TX_INVALID &&
                  CV_NS_BAD_KEY == CVN_BAD_KEY && CV_NS_SIGNATURES_MISSING == CVN_SIGNATURES_MISSING &&
                  CV_NS_MALFORMED == CVN_MALFORMED && CV_NS_CONFLICT == CVN_CONFLICT && CV_VS_MISSING == CVN_VS_MISSING &&
                  CV_VS_MALFORMED == CVN_VS_MALFORMED && CV_UNIQ_CONFLICT == CVN_UNIQ_CONFLICT &&
                  CV_SIG_BAD_KEY == CVN_SIG_BAD_KEY && CVN_D_ACCEPTED > CVU_D_BAD && CVN_D_ACCEPTED < CVU_D_ROUND0,
              "cv_notary.h, cv_uniq.h and the public header agree");

// begin[0] == 0 and monotone; the last entry is the count
static bool ranges_ok(const uint32_t *begin, size_t n) {
    if (begin[0] != 0) return false;
    for (size_t i = 0; i < n; i++)
        if (begin[i + 1] < begin[i]) return false;
    return true;
}

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
        if (!ranges_ok(tx_req_begin, T) || tx_req_begin[T] != nreq || !ranges_ok(req_begin, nreq) || req_begin[nreq] != nnodes)
            return CV_E_ARGS;
        if (nnodes && (!kind || !leaf_key || !threshold || !child_begin)) return CV_E_ARGS;
        if (nchild && (!child || !weight)) return CV_E_ARGS;
        if (nnodes ? (child_begin[0] != 0 || child_begin[nnodes] != nchild) : nchild != 0) return CV_E_ARGS;
    }
    // the leaves' extent: a record past the arena, or one whose off + len wraps, fails before any copy or launch
    uint64_t lo = UINT64_MAX, hi = 0;
    for (size_t i = 0; i < L; i++) {
        const uint64_t end = leaf_off[i] + leaf_len[i];
        if (end < leaf_off[i] || end > leaf_arena_bytes) return CV_E_ARGS;
        lo = std::min(lo, leaf_off[i]);
        hi = std::max(hi, end);
    }
    if (hi < lo) lo = hi = 0;
    if (hi > lo && !leaf_arena) return CV_E_ARGS;
    if (!ctx || !u || !sg || u->ctx != ctx || sg->ctx != ctx) return CV_E_ARGS;
    size_t dev = ctx->devs.size();
    for (size_t k = 0; k < ctx->devs.size(); k++)
        if (ctx->devs[k]->ordinal == u->ordinal) dev = k;
    if (dev == ctx->devs.size() || dev >= sg->rec.size() || !sg->rec[dev]) return CV_E_ARGS;

    std::lock_guard<std::mutex> g(u->mu);
    if (u->resident + S > u->capacity) return CV_E_OOM;          // before any change and any output
    CV_TRY(hipSetDevice(u->ordinal));
    // inputs (one upload) | workspace | outputs (one read-back), every piece 16-byte aligned
    size_t top = 0;
    auto take = [&top](size_t bytes) {
        const size_t at = top;
        top += al16(bytes);
        return at;
    };
    const size_t R = nreq, W = (N + 63) / 64, bs = (size_t)uniq_bmask(S) + 1;
    const size_t i_arena = take(hi - lo), i_loff = take(8 * L), i_llen = take(4 * L), i_txb = take(4 * (T + 1));
    const size_t i_claim = take(32 * T), i_cal = take(4 * T), i_tpre = take(T), i_sbeg = take(4 * (T + 1));
    const size_t i_sleaf = take(4 * S), i_pk = take(32 * N), i_sig = take(64 * N), i_tsb = take(val ? 4 * (T + 1) : 0);
    const size_t i_spre = take(N), i_kind = take(nnodes), i_lkey = take(32 * nnodes), i_thr = take(4 * nnodes);
    const size_t i_cb = take(val ? 4 * (nnodes + 1) : 0), i_child = take(4 * nchild), i_w = take(4 * nchild);
    const size_t i_rb = take(val ? 4 * (R + 1) : 0), i_trb = take(val ? 4 * (T + 1) : 0), i_skey = take(32 * N);
    const size_t i_allow = take(R), in_bytes = top;
    const size_t w_ldig = take(32 * L), w_mst = take(T), w_voff = take(8 * N), w_vlen = take(4 * N), w_bm = take(8 * W);
    const size_t w_sst = take(N), w_ck = take(val ? (size_t)cvck_ws_bytes(T, nnodes) : 0), w_ckst = take(T);
    const size_t w_pre = take(T), w_en = take(T), w_key = take(32 * S), w_bt = take(4 * bs), w_rep = take(4 * S);
    const size_t w_res = take(4 * S), w_stx = take(4 * S), w_own = take(4 * S), w_last = take(4 * S), w_s0 = take(4 * T);
    const size_t w_s1 = take(4 * T), w_ust = take(T), w_list = take(4 * T), w_soff = take(8 * T), w_slen = take(4 * T);
    const size_t w_csig = take(64 * T);
    const size_t o_out = take(T), o_ids = take(32 * T), o_fb = take(4 * T), o_miss = take(R), o_sc = take(S);
    const size_t o_cid = take(32 * S), o_cix = take(4 * S), o_cc = take(4 * S), o_nsig = take(64 * T);
    const size_t out_bytes = top - o_out, total = top + 16;
    CV_TRY(u->nin.ensure(in_bytes + 16));
    CV_TRY(u->nout.ensure(out_bytes + 16));
    CV_TRY(u->nws.ensure(total));

    // pack: the leaf offsets rebased to the copied part of the arena; the states' prefix sum and leaf indices
    uint8_t *h = u->nin.as<uint8_t>();
    struct Piece {
        uint8_t *dst;
        const uint8_t *src;
        size_t bytes;
    };
    std::vector<Piece> pieces;
    auto put = [h, &pieces](size_t at, const void *src, size_t bytes) {
        if (bytes) pieces.push_back({h + at, static_cast<const uint8_t *>(src), bytes});
    };
    put(i_arena, leaf_arena ? leaf_arena + lo : nullptr, hi - lo);
    uint64_t *hoff = reinterpret_cast<uint64_t *>(h + i_loff);
    for (size_t i = 0; i < L; i++) hoff[i] = leaf_off[i] - lo;
    put(i_llen, leaf_len, 4 * L);
    put(i_txb, tx_leaf_begin, 4 * (T + 1));
    put(i_claim, claimed_id, 32 * T);
    put(i_cal, caller, 4 * T);
    if (tx_pre) put(i_tpre, tx_pre, T);
    uint32_t *hsb = reinterpret_cast<uint32_t *>(h + i_sbeg), *hsl = reinterpret_cast<uint32_t *>(h + i_sleaf);
    size_t at = 0;
    for (size_t t = 0; t < T; t++) {
        hsb[t] = (uint32_t)at;
        for (uint32_t j = 0; j < tx_input_count[t]; j++) hsl[at++] = tx_leaf_begin[t] + j;
    }
    hsb[T] = (uint32_t)at;
    if (val) {
        put(i_pk, pk, 32 * N);
        put(i_sig, sig, 64 * N);
        put(i_tsb, tx_sig_begin, 4 * (T + 1));
        if (sig_pre) put(i_spre, sig_pre, N);
        put(i_kind, kind, nnodes);
        put(i_lkey, leaf_key, 32 * nnodes);
        put(i_thr, threshold, 4 * nnodes);
        if (nnodes) put(i_cb, child_begin, 4 * (nnodes + 1));
        put(i_child, child, 4 * nchild);
        put(i_w, weight, 4 * nchild);
        put(i_rb, req_begin, 4 * (R + 1));
        put(i_trb, tx_req_begin, 4 * (T + 1));
        put(i_skey, sig_key, 32 * N);
        if (req_allowed) put(i_allow, req_allowed, R);
    }

    // the copies: one after another for a notary-sized batch, cut into 256 KB tasks over the set's host threads
    // (CV_OPT_HOST_THREADS, as the verify pipeline packs pageable inputs) from 4 MB up
    size_t pack_bytes = 0;
    for (const Piece &pc : pieces) pack_bytes += pc.bytes;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int threads = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->opt[CV_OPT_HOST_THREADS].load(), hw));
    if (pack_bytes < ((size_t)4 << 20) || threads == 1) {
        for (const Piece &pc : pieces) std::memcpy(pc.dst, pc.src, pc.bytes);
    } else {
        if (!u->pool || u->pool->threads() != threads) u->pool.reset(new WorkerPool(threads - 1));
        const size_t cut = (size_t)256 << 10;
        std::vector<Piece> tasks;
        for (const Piece &pc : pieces)
            for (size_t at = 0; at < pc.bytes; at += cut) tasks.push_back({pc.dst + at, pc.src + at, std::min(cut, pc.bytes - at)});
        u->pool->run(tasks.size(), [&tasks](size_t i) { std::memcpy(tasks[i].dst, tasks[i].src, tasks[i].bytes); });
    }

    uint8_t *base = u->nws.as<uint8_t>();
    auto u32 = [base](size_t off) { return reinterpret_cast<uint32_t *>(base + off); };
    auto i32 = [base](size_t off) { return reinterpret_cast<int32_t *>(base + off); };
    auto u64 = [base](size_t off) { return reinterpret_cast<uint64_t *>(base + off); };
    hipStream_t s = u->stream;
    auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });
    int rc = uniq_stat_begin(u);
    if (rc != CV_OK) return rc;
    CV_TRY(hipMemcpyAsync(base, h, in_bytes, hipMemcpyHostToDevice, s));

    CvNotary Q{};
    Q.ntx = (uint32_t)T, Q.nstates = (uint32_t)S, Q.validating = val ? 1 : 0;
    Q.mstatus = base + w_mst, Q.id = u32(o_ids), Q.claimed = u32(i_claim), Q.tx_pre = tx_pre ? base + i_tpre : nullptr;
    Q.tx_sig_begin = u32(i_tsb), Q.bitmap = u64(w_bm), Q.sig_status = base + w_sst;
    Q.sig_pre = val && sig_pre ? base + i_spre : nullptr, Q.ck_status = base + w_ckst;
    Q.pre = base + w_pre, Q.enable = base + w_en, Q.first_bad = u32(o_fb);
    Q.leaf_digest = u32(w_ldig), Q.state_leaf = u32(i_sleaf), Q.key = u32(w_key);
    Q.uniq_status = base + w_ust, Q.outcome = base + o_out;
    Q.list = u32(w_list), Q.sign_off = u64(w_soff), Q.sign_len = u32(w_slen);

    // leaf hashes, the state keys out of them, then the trees (which fold the digests in place)
    CV_TRY(cvk_merkle(0, (uint32_t)L, 0, base + i_arena, u64(i_loff), u32(i_llen), u32(i_txb), u32(w_ldig), nullptr,
                      nullptr, s));
    CV_TRY(cvk_notary_gather(&Q, s));
    CV_TRY(cvk_merkle((uint32_t)T, 0, 0, base + i_arena, u64(i_loff), u32(i_llen), u32(i_txb), u32(w_ldig), base + o_ids,
                      base + w_mst, s));
    if (val) {
        if (N) {
            CV_TRY(cvk_tx_sig_refs((uint32_t)N, 0, (uint32_t)T, 0, u32(i_tsb), u64(w_voff), u32(w_vlen), s));
            rc = cv_ed25519_verify_device(ctx, u->ordinal, N, base + i_pk, base + i_sig, base + o_ids, base + w_voff,
                                          base + w_vlen, base + w_bm, base + w_sst, s);
            if (rc != CV_OK) return rc;
        }
        CvCk a{};
        a.ntx = (uint32_t)T, a.nreq = (uint32_t)R, a.nnodes = (uint32_t)nnodes, a.nchild = (uint32_t)nchild;
        a.nsig = (uint32_t)N;
        a.kind = base + i_kind, a.leaf_key = base + i_lkey, a.threshold = i32(i_thr), a.child_begin = u32(i_cb);
        a.child = u32(i_child), a.weight = i32(i_w), a.req_begin = u32(i_rb), a.tx_req_begin = u32(i_trb);
        a.sig_key = base + i_skey, a.tx_sig_begin = u32(i_tsb);
        a.req_allowed = req_allowed ? base + i_allow : nullptr;
        a.bitmap = N ? u64(w_bm) : nullptr;
        a.wide_min = 0;
        a.count = u32(w_ck), a.list = u32(w_ck + CVCK_WS_LIST), a.flag = base + w_ck + cvck_ws_flag_off(T);
        a.req_missing = base + o_miss, a.tx_status = base + w_ckst;
        CV_TRY(cvk_ck(&a, s));
    }
    CV_TRY(cvk_notary_gate(&Q, s));
    // records of states without a conflict and signatures of transactions that are not committed: zero
    CV_TRY(hipMemsetAsync(base + o_cid, 0, o_nsig + al16(64 * T) - o_cid, s));
    CvUniqBatch B{};
    B.ntx = (uint32_t)T, B.nstates = (uint32_t)S;
    B.key = u32(w_key), B.begin = u32(i_sbeg), B.id = u32(o_ids), B.caller = u32(i_cal), B.enable = base + w_en;
    B.btab = u32(w_bt), B.bmask = (uint32_t)(bs - 1);
    B.rep = u32(w_rep), B.res = u32(w_res), B.state_tx = u32(w_stx), B.owner = u32(w_own), B.last = u32(w_last);
    B.tx_status = base + w_ust, B.state_conflict = base + o_sc;
    B.cons_id = u32(o_cid), B.cons_index = u32(o_cix), B.cons_caller = u32(o_cc);
    B.dstat = u->dstat.as<uint32_t>();
    uint64_t rounds = 0;
    rc = uniq_decide(u, B, u32(w_s0), u32(w_s1), &rounds);
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
    CV_TRY(cvk_sign_keyed(count, static_cast<const uint32_t *>(sg->rec[dev]), base + o_ids, u64(w_soff), u32(w_slen),
                          base + w_csig, s));
    CV_TRY(cvk_notary_scatter(count, u32(w_list), base + w_csig, base + o_nsig, s));
    uint8_t *ho = u->nout.as<uint8_t>();
    CV_TRY(hipMemcpyAsync(ho, base + o_out, out_bytes, hipMemcpyDeviceToHost, s));
    CV_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    auto get = [ho, o_out](void *dst, size_t off, size_t bytes) {
        if (dst && bytes) std::memcpy(dst, ho + (off - o_out), bytes);
    };
    get(outcome, o_out, T);
    get(ids, o_ids, 32 * T);
    get(first_bad, o_fb, 4 * T);
    get(req_missing, o_miss, R);
    get(state_conflict, o_sc, S);
    get(consumed_id, o_cid, 32 * S);
    get(consumed_index, o_cix, 4 * S);
    get(consumed_caller, o_cc, 4 * S);
    get(notary_sig, o_nsig, 64 * T);
    return CV_OK;
}

}  // extern "C"
