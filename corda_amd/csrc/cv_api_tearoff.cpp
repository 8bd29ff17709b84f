// cv_api_tearoff.cpp — the verifier side of a tear-off and the oracle's signing step of the C-ABI
// (include/cordaverify.h): cv_filtered_verify and cv_tearoff_sign_batch.  The decisions between the stages are
// cv_tearoff.h's; the signer and the engine state are cv_host.h's.
//
// One device, the least loaded (tear-off batches are small), everything in d.pmt on d.stream: ONE upload of the
// inputs (packed in pinned memory), leaf hashes -> check bytes -> tree verify (the filtered leaves' digests as its
// check hashes, tx_leaf_begin as its check ranges) -> gate; the signing call goes on with the ordered compaction, the
// signing of the accepted roots into a compact array and their scatter.  ONE read-back of the outputs (through pinned
// memory); the signing call synchronises once more before it, for the accepted count.
#include "cv_host.h"

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

// begin[0] == 0 and monotone; the last entry is the count
bool ranges_ok(const uint32_t *begin, size_t n) {
    if (begin[0] != 0) return false;
    for (size_t i = 0; i < n; i++)
        if (begin[i + 1] < begin[i]) return false;
    return true;
}

// The checks both calls share, all before any device work (the callers test the counts and their outputs before, the
// context after): the ranges well formed, every leaf inside the arena, leaf_pre within its codes.  lo, hi: the part
// of the arena the leaves reach.
int ts_check(const TsIn &in, uint64_t *lo, uint64_t *hi) {
    if (!in.txb || !in.tree_begin || !in.root) return CV_E_ARGS;
    if (in.nnodes && (!in.kind || !in.left || !in.right || !in.node_hash)) return CV_E_ARGS;
    if (!ranges_ok(in.txb, in.ntx) || !ranges_ok(in.tree_begin, in.ntx) || in.tree_begin[in.ntx] != in.nnodes)
        return CV_E_ARGS;
    const size_t L = in.txb[in.ntx];
    if (L > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (L && (!in.off || !in.len)) return CV_E_ARGS;
    uint64_t a = UINT64_MAX, b = 0;
    for (size_t i = 0; i < L; i++) {
        const uint64_t end = in.off[i] + in.len[i];
        if (end < in.off[i] || end > in.arena_bytes) return CV_E_ARGS;   // wraps, or past the arena
        a = std::min(a, in.off[i]);
        b = std::max(b, end);
    }
    if (b < a) a = b = 0;
    if (b > a && !in.arena) return CV_E_ARGS;
    if (in.leaf_pre)
        for (size_t i = 0; i < L; i++)
            if (in.leaf_pre[i] > CVT_PRE_UNKNOWN) return CV_E_ARGS;
    *lo = a;
    *hi = b;
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
    Opts o = ctx->opts();
    o.shard_min = o.spread_min = SIZE_MAX;   // one device, the least loaded
    return dispatch(ctx, o, in.ntx, 1, [&](Device &d, size_t, size_t, int threads) {
        // the signer's record for this device, by ordinal
        size_t dev = ctx->devs.size();
        for (size_t k = 0; k < ctx->devs.size(); k++)
            if (ctx->devs[k]->ordinal == d.ordinal) dev = k;
        if (sg && (dev >= sg->rec.size() || !sg->rec[dev])) return (int)CV_E_ARGS;
        CV_TRY(hipSetDevice(d.ordinal));
        const size_t T = in.ntx, L = in.txb[T], M = in.nnodes;
        const bool sign = sg != nullptr;
        // inputs (one upload) | workspace | outputs (one read-back), every piece 16-byte aligned
        size_t top = 0;
        auto take = [&top](size_t bytes) {
            const size_t at = top;
            top += al16(bytes);
            return at;
        };
        const size_t i_arena = take(hi - lo), i_loff = take(8 * L), i_llen = take(4 * L), i_txb = take(4 * (T + 1));
        const size_t i_kind = take(M), i_left = take(4 * M), i_right = take(4 * M), i_hash = take(32 * M);
        const size_t i_tb = take(4 * (T + 1)), i_root = take(32 * T), i_pre = take(in.leaf_pre ? L : 0);
        const size_t in_bytes = top;
        const size_t w_ldig = take(32 * L), w_check = take(32 * L), w_dig = take(32 * M), w_flag = take(M + 1);
        const size_t w_v = take(T), w_st = take(T), w_list = take(sign ? 4 * T : 0), w_soff = take(sign ? 8 * T : 0);
        const size_t w_slen = take(sign ? 4 * T : 0), w_csig = take(sign ? 64 * T : 0);
        const size_t o_cnt = take(16), o_out = take(T), o_fb = take(4 * T), o_fv = take(T), o_fst = take(T);
        const size_t o_sig = take(sign ? 64 * T : 0);
        const size_t out_bytes = top - o_cnt, total = top + 16;
        CV_TRY(d.ts_in.ensure(in_bytes + 16));
        CV_TRY(d.ts_out.ensure(out_bytes + 16));
        CV_TRY(d.pmt.ensure(total));

        // pack: the leaf offsets rebased to the copied part of the arena
        uint8_t *h = d.ts_in.as<uint8_t>();
        struct Piece {
            uint8_t *dst;
            const uint8_t *src;
            size_t bytes;
        };
        std::vector<Piece> pieces;
        auto put = [h, &pieces](size_t at, const void *src, size_t bytes) {
            if (bytes) pieces.push_back({h + at, static_cast<const uint8_t *>(src), bytes});
        };
        put(i_arena, in.arena ? in.arena + lo : nullptr, hi - lo);
        uint64_t *hoff = reinterpret_cast<uint64_t *>(h + i_loff);
        for (size_t i = 0; i < L; i++) hoff[i] = in.off[i] - lo;
        put(i_llen, in.len, 4 * L);
        put(i_txb, in.txb, 4 * (T + 1));
        put(i_kind, in.kind, M);
        put(i_left, in.left, 4 * M);
        put(i_right, in.right, 4 * M);
        put(i_hash, in.node_hash, 32 * M);
        put(i_tb, in.tree_begin, 4 * (T + 1));
        put(i_root, in.root, 32 * T);
        if (in.leaf_pre) put(i_pre, in.leaf_pre, L);
        // the copies: one after another for an oracle-sized batch, cut into 256 KB tasks over the device's host threads
        // (CV_OPT_HOST_THREADS) from 4 MB up, as cv_notarise_batch packs its inputs
        size_t pack_bytes = 0;
        for (const Piece &pc : pieces) pack_bytes += pc.bytes;
        if (pack_bytes < ((size_t)4 << 20) || threads == 1) {
            for (const Piece &pc : pieces) std::memcpy(pc.dst, pc.src, pc.bytes);
        } else {
            const size_t cut = (size_t)256 << 10;
            std::vector<Piece> tasks;
            for (const Piece &pc : pieces)
                for (size_t at = 0; at < pc.bytes; at += cut) tasks.push_back({pc.dst + at, pc.src + at, std::min(cut, pc.bytes - at)});
            d.workers(threads).run(tasks.size(), [&tasks](size_t i) { std::memcpy(tasks[i].dst, tasks[i].src, tasks[i].bytes); });
        }

        uint8_t *base = d.pmt.as<uint8_t>();
        auto u32 = [base](size_t off) { return reinterpret_cast<uint32_t *>(base + off); };
        auto u64 = [base](size_t off) { return reinterpret_cast<uint64_t *>(base + off); };
        hipStream_t s = d.stream;
        auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });
        CV_TRY(hipMemcpyAsync(base, h, in_bytes, hipMemcpyHostToDevice, s));

        CvTearoff Q{};
        Q.ntx = (uint32_t)T, Q.nleaves = (uint32_t)L;
        Q.leaf_digest = u32(w_ldig), Q.check = u32(w_check);
        Q.tx_leaf_begin = u32(i_txb), Q.verdict = base + w_v, Q.status = base + w_st;
        Q.leaf_pre = in.leaf_pre ? base + i_pre : nullptr;
        Q.fv_verdict = base + o_fv, Q.fv_status = base + o_fst;
        Q.outcome = base + o_out, Q.first_bad = u32(o_fb);
        Q.list = u32(w_list), Q.sign_off = u64(w_soff), Q.sign_len = u32(w_slen);

        // the leaf kernel alone (no transactions), then its digests as the bytes the tree verify compares
        CV_TRY(cvk_merkle(0, (uint32_t)L, 0, base + i_arena, u64(i_loff), u32(i_llen), u32(i_txb), u32(w_ldig), nullptr,
                          nullptr, s));
        CV_TRY(cvk_tearoff_check(&Q, s));
        CV_TRY(cvk_pmt_verify((uint32_t)T, base + i_kind, u32(i_left), u32(i_right), base + i_hash, u32(i_tb), base + i_root,
                              base + w_check, u32(i_txb), u32(w_dig), base + w_flag, base + w_v, base + w_st, s));
        CV_TRY(cvk_tearoff_gate(&Q, s));
        uint8_t *ho = d.ts_out.as<uint8_t>();
        if (sign) {
            // signatures of tear-offs that are refused: zero
            CV_TRY(hipMemsetAsync(base + o_sig, 0, al16(64 * T), s));
            CV_TRY(cvk_tearoff_compact(&Q, u32(o_cnt), s));
            CV_TRY(hipMemcpyAsync(ho, base + o_cnt, 16, hipMemcpyDeviceToHost, s));
            CV_TRY(hipStreamSynchronize(s));                         // the accepted count is on the host
            const uint32_t count = *reinterpret_cast<const uint32_t *>(ho);
            if (count > T) {
                drain.armed = false;
                return (int)CV_E_HIP;
            }
            // the signing kernel runs for the accepted tear-offs alone, into a compact array; the scatter places them
            CV_TRY(cvk_sign_keyed(count, static_cast<const uint32_t *>(sg->rec[dev]), base + i_root, u64(w_soff),
                                  u32(w_slen), base + w_csig, s));
            CV_TRY(cvk_notary_scatter(count, u32(w_list), base + w_csig, base + o_sig, s));
        }
        CV_TRY(hipMemcpyAsync(ho, base + o_cnt, out_bytes, hipMemcpyDeviceToHost, s));
        CV_TRY(hipStreamSynchronize(s));
        drain.armed = false;
        auto get = [ho, o_cnt](void *dst, size_t off, size_t bytes) {
            if (dst && bytes) std::memcpy(dst, ho + (off - o_cnt), bytes);
        };
        get(out.verdict, o_fv, T);
        get(out.status, o_fst, T);
        get(out.outcome, o_out, T);
        get(out.first_bad, o_fb, 4 * T);
        if (sign) get(out.sig, o_sig, 64 * T);
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
