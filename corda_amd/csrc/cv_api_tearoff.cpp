// cv_api_tearoff.cpp — the verifier side of a tear-off and the oracle's signing step of the C-ABI
// (include/cordaverify.h): cv_filtered_verify and cv_tearoff_sign_batch.  The decisions between the stages are
// cv_tearoff.h's; the signer and the engine state are cv_host.h's.
//
// One device, the least loaded (tear-off batches are small), everything in d.pmt on d.stream: ONE upload of the
// inputs (packed in pinned memory), leaf hashes -> check bytes -> tree verify (the filtered leaves' digests as its
// check hashes, tx_leaf_begin as its check ranges) -> gate; the signing call goes on with the ordered compaction, the
// signing of the accepted roots into a compact array and their scatter.  ONE read-back of the outputs (through pinned
// memory); the signing call synchronises once more before it, for the accepted count.  The checks of the ranges and the
// leaves, the buffer's layout, the pack list and the read-back are cv_batch.h's.
#include "cv_batch.h"

using namespace cvh;

static_assert(CV_TS_SUCCESS == CVT_SUCCESS && CV_TS_NO_LEAVES == CVT_NO_LEAVES && CV_TS_MALFORMED == CVT_MALFORMED &&
                  CV_TS_VERIFY_FAILED == CVT_VERIFY_FAILED && CV_TS_NOT_COMMANDS == CVT_NOT_COMMANDS &&
                  CV_TS_WRONG_COMMAND == CVT_WRONG_COMMAND && CV_TS_UNKNOWN == CVT_UNKNOWN &&
                  CV_TS_NOT_COMMANDS == CV_TS_VERIFY_FAILED + CVT_PRE_NOT_COMMAND &&
                  CV_TS_UNKNOWN == CV_TS_VERIFY_FAILED + CVT_PRE_UNKNOWN && CV_PMT_OK == CVT_PMT_OK &&
                  CV_PMT_MALFORMED == CVT_PMT_MALFORMED && CV_PMT_NO_INCLUDED == CVT_PMT_NO_INCLUDED,
              "cv_tearoff.h and the public header agree");

namespace {

struct TsIn {
    size_t ntx;
    const uint8_t *arena;
    uint64_t arena_bytes;
    const uint64_t *off;
    const uint32_t *len;
    const uint32_t *txb;
    size_t nnodes;
    const uint8_t *kind;
    const uint32_t *left, *right;
    const uint8_t *node_hash;
    const uint32_t *tree_begin;
    const uint8_t *root;
    const uint8_t *leaf_pre;           // the signing call only
};

// The checks both calls share, all before any device work (the callers test the counts and their outputs before, the
// context after): the ranges well formed, every leaf inside the arena, leaf_pre within its codes.  lo, hi: the part
// of the arena the leaves reach.
int ts_check(const TsIn &in, uint64_t *lo, uint64_t *hi) {
    if (!in.txb || !in.tree_begin || !in.root) return CV_E_ARGS;
    if (in.nnodes && (!in.kind || !in.left || !in.right || !in.node_hash)) return CV_E_ARGS;
    if (!ranges_ok(in.txb, in.ntx) || !ranges_ok(in.tree_begin, in.ntx, in.nnodes)) return CV_E_ARGS;
    const size_t L = in.txb[in.ntx];
    if (L > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (L && (!in.off || !in.len)) return CV_E_ARGS;
    const Extent ext = arena_extent(0, L, in.off, in.len, in.arena_bytes);   // a wrapping record is out of bounds too
    if (!ext.ok || (ext.hi > ext.lo && !in.arena)) return CV_E_ARGS;
    if (in.leaf_pre)
        for (size_t i = 0; i < L; i++)
            if (in.leaf_pre[i] > CVT_PRE_UNKNOWN) return CV_E_ARGS;
    *lo = ext.lo;
    *hi = ext.hi;
    return CV_OK;
}

struct TsOut {
    uint8_t *verdict, *status;         // cv_filtered_verify
    uint8_t *outcome;                  // cv_tearoff_sign_batch
    uint32_t *first_bad;
    uint8_t *sig;
};

// sg == nullptr: the verify alone (verdict, status); else the oracle's step with that signer (outcome, first_bad, sig)
int ts_run(cv_ctx *ctx, const cv_signer *sg, const TsIn &in, uint64_t lo, uint64_t hi, const TsOut &out) {
    return dispatch_one(ctx, in.ntx, [&](Device &d, size_t, size_t, int threads) {
        const uint32_t *rec = sg ? signer_rec(sg, d) : nullptr;
        if (sg && !rec) return (int)CV_E_ARGS;
        CV_TRY(hipSetDevice(d.ordinal));
        const size_t T = in.ntx, L = in.txb[T], M = in.nnodes;
        const bool sign = sg != nullptr;
        // inputs (one upload) | workspace | outputs (one read-back)
        Layout lay;
        const size_t i_arena = lay.take(hi - lo), i_loff = lay.take(8 * L), i_llen = lay.take(4 * L);
        const size_t i_txb = lay.take(4 * (T + 1)), i_kind = lay.take(M), i_left = lay.take(4 * M);
        const size_t i_right = lay.take(4 * M), i_hash = lay.take(32 * M), i_tb = lay.take(4 * (T + 1));
        const size_t i_root = lay.take(32 * T), i_pre = lay.take(in.leaf_pre ? L : 0), in_bytes = lay.top;
        const size_t w_ldig = lay.take(32 * L), w_check = lay.take(32 * L), w_dig = lay.take(32 * M);
        const size_t w_flag = lay.take(M + 1), w_v = lay.take(T), w_st = lay.take(T), w_list = lay.take(sign ? 4 * T : 0);
        const size_t w_soff = lay.take(sign ? 8 * T : 0), w_slen = lay.take(sign ? 4 * T : 0);
        const size_t w_csig = lay.take(sign ? 64 * T : 0);
        const size_t o_cnt = lay.take(16), o_out = lay.take(T), o_fb = lay.take(4 * T), o_fv = lay.take(T);
        const size_t o_fst = lay.take(T), o_sig = lay.take(sign ? 64 * T : 0);
        const size_t out_bytes = lay.top - o_cnt, total = lay.top + 16;
        CV_TRY(d.ts_in.ensure(in_bytes + 16));
        CV_TRY(d.ts_out.ensure(out_bytes + 16));
        CV_TRY(d.pmt.ensure(total));

        // pack: the leaf offsets rebased to the copied part of the arena
        uint8_t *h = d.ts_in.as<uint8_t>();
        Pack pk{h};
        pk.put(i_arena, in.arena ? in.arena + lo : nullptr, hi - lo);
        uint64_t *hoff = at<uint64_t>(h, i_loff);
        for (size_t i = 0; i < L; i++) hoff[i] = in.off[i] - lo;
        pk.put(i_llen, in.len, 4 * L);
        pk.put(i_txb, in.txb, 4 * (T + 1));
        pk.put(i_kind, in.kind, M);
        pk.put(i_left, in.left, 4 * M);
        pk.put(i_right, in.right, 4 * M);
        pk.put(i_hash, in.node_hash, 32 * M);
        pk.put(i_tb, in.tree_begin, 4 * (T + 1));
        pk.put(i_root, in.root, 32 * T);
        if (in.leaf_pre) pk.put(i_pre, in.leaf_pre, L);
        // the copies, from 4 MB up over the device's host threads (CV_OPT_HOST_THREADS), as cv_notarise_batch's
        pk.run(pk.wants_pool(threads) ? &d.workers(threads) : nullptr);

        uint8_t *base = d.pmt.as<uint8_t>();
        hipStream_t s = d.stream;
        auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });
        CV_TRY(hipMemcpyAsync(base, h, in_bytes, hipMemcpyHostToDevice, s));

        uint32_t *const d_txb = at<uint32_t>(base, i_txb);
        CvTearoff Q{};
        Q.ntx = (uint32_t)T, Q.nleaves = (uint32_t)L;
        Q.leaf_digest = at<uint32_t>(base, w_ldig), Q.check = at<uint32_t>(base, w_check);
        Q.tx_leaf_begin = d_txb, Q.verdict = base + w_v, Q.status = base + w_st;
        Q.leaf_pre = in.leaf_pre ? base + i_pre : nullptr;
        Q.fv_verdict = base + o_fv, Q.fv_status = base + o_fst;
        Q.outcome = base + o_out, Q.first_bad = at<uint32_t>(base, o_fb), Q.list = at<uint32_t>(base, w_list);
        Q.sign_off = at<uint64_t>(base, w_soff), Q.sign_len = at<uint32_t>(base, w_slen);

        // the leaf kernel alone (no transactions), then its digests as the bytes the tree verify compares
        CV_TRY(cvk_merkle(0, (uint32_t)L, 0, base + i_arena, at<uint64_t>(base, i_loff), at<uint32_t>(base, i_llen), d_txb,
                          at<uint32_t>(base, w_ldig), nullptr, nullptr, s));
        CV_TRY(cvk_tearoff_check(&Q, s));
        CV_TRY(cvk_pmt_verify((uint32_t)T, base + i_kind, at<uint32_t>(base, i_left), at<uint32_t>(base, i_right),
                              base + i_hash, at<uint32_t>(base, i_tb), base + i_root, base + w_check, d_txb,
                              at<uint32_t>(base, w_dig), base + w_flag, base + w_v, base + w_st, s));
        CV_TRY(cvk_tearoff_gate(&Q, s));
        uint8_t *ho = d.ts_out.as<uint8_t>();
        if (sign) {
            // signatures of tear-offs that are refused: zero
            CV_TRY(hipMemsetAsync(base + o_sig, 0, al16(64 * T), s));
            CV_TRY(cvk_tearoff_compact(&Q, at<uint32_t>(base, o_cnt), s));
            CV_TRY(hipMemcpyAsync(ho, base + o_cnt, 16, hipMemcpyDeviceToHost, s));
            CV_TRY(hipStreamSynchronize(s));                         // the accepted count is on the host
            const uint32_t count = *at<uint32_t>(ho, 0);
            if (count > T) {
                drain.armed = false;
                return (int)CV_E_HIP;
            }
            // the signing kernel runs for the accepted tear-offs alone, into a compact array; the scatter places them
            CV_TRY(cvk_sign_keyed(count, rec, base + i_root, Q.sign_off, Q.sign_len, base + w_csig, s));
            CV_TRY(cvk_notary_scatter(count, Q.list, base + w_csig, base + o_sig, s));
        }
        CV_TRY(hipMemcpyAsync(ho, base + o_cnt, out_bytes, hipMemcpyDeviceToHost, s));
        CV_TRY(hipStreamSynchronize(s));
        drain.armed = false;
        const Unpack res{ho, o_cnt};
        res.get(out.verdict, o_fv, T);
        res.get(out.status, o_fst, T);
        res.get(out.outcome, o_out, T);
        res.get(out.first_bad, o_fb, 4 * T);
        if (sign) res.get(out.sig, o_sig, 64 * T);
        return (int)CV_OK;
    });
}

}  // namespace

extern "C" {

int cv_filtered_verify(cv_ctx *ctx, size_t ntx, const uint8_t *leaf_arena, uint64_t leaf_arena_bytes,
                       const uint64_t *leaf_off, const uint32_t *leaf_len, const uint32_t *tx_leaf_begin, size_t nnodes,
                       const uint8_t *kind, const uint32_t *left, const uint32_t *right, const uint8_t *node_hash,
                       const uint32_t *tree_begin, const uint8_t *root, uint8_t *verdict, uint8_t *status) {
    if (ntx == 0) return CV_OK;
    const TsIn in{ntx, leaf_arena, leaf_arena_bytes, leaf_off, leaf_len, tx_leaf_begin, nnodes, kind, left, right,
                  node_hash, tree_begin, root, nullptr};
    if (ntx > 0xfffffffeull || nnodes > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (!verdict) return CV_E_ARGS;
    uint64_t lo = 0, hi = 0;
    const int rc = ts_check(in, &lo, &hi);
    if (rc != CV_OK) return rc;
    if (!ctx) return CV_E_ARGS;
    return ts_run(ctx, nullptr, in, lo, hi, TsOut{verdict, status, nullptr, nullptr, nullptr});
}

int cv_tearoff_sign_batch(cv_ctx *ctx, const cv_signer *s, size_t ntx, const uint8_t *leaf_arena,
                          uint64_t leaf_arena_bytes, const uint64_t *leaf_off, const uint32_t *leaf_len,
                          const uint32_t *tx_leaf_begin, size_t nnodes, const uint8_t *kind, const uint32_t *left,
                          const uint32_t *right, const uint8_t *node_hash, const uint32_t *tree_begin, const uint8_t *root,
                          const uint8_t *leaf_pre, uint8_t *outcome, uint32_t *first_bad, uint8_t *sig_out) {
    if (ntx == 0) return CV_OK;
    const TsIn in{ntx, leaf_arena, leaf_arena_bytes, leaf_off, leaf_len, tx_leaf_begin, nnodes, kind, left, right,
                  node_hash, tree_begin, root, leaf_pre};
    if (ntx > 0xfffffffeull || nnodes > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (!outcome || !sig_out) return CV_E_ARGS;
    uint64_t lo = 0, hi = 0;
    const int rc = ts_check(in, &lo, &hi);
    if (rc != CV_OK) return rc;
    if (!ctx || !s || s->ctx != ctx) return CV_E_ARGS;
    return ts_run(ctx, s, in, lo, hi, TsOut{nullptr, nullptr, outcome, first_bad, sig_out});
}

}  // extern "C"
