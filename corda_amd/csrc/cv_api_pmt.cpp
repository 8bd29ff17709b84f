// cv_api_pmt.cpp — partial Merkle trees (tear-offs) of the C-ABI (include/cordaverify.h): cv_partial_merkle_verify
// and the builds, cv_partial_merkle_build and cv_filtered_build.  The engine state is cv_host.h's; the range checks,
// the buffer's layout and the routing to one device are cv_batch.h's.
#include "cv_batch.h"

using namespace cvh;

extern "C" {

int cv_partial_merkle_verify(cv_ctx *ctx, size_t ntrees, size_t nnodes, const uint8_t *kind, const uint32_t *left,
                             const uint32_t *right, const uint8_t *leaf_hash, const uint32_t *tree_begin,
                             const uint8_t *root, size_t ncheck, const uint8_t *check, const uint32_t *check_begin,
                             uint8_t *verdict, uint8_t *status) {
    if (!ctx) return CV_E_ARGS;
    if (ntrees == 0) return CV_OK;
    if (!tree_begin || !check_begin || !root || !verdict) return CV_E_ARGS;
    if (nnodes && (!kind || !left || !right || !leaf_hash)) return CV_E_ARGS;
    if (ncheck && !check) return CV_E_ARGS;
    if (ntrees > 0xfffffffeull || nnodes > 0xfffffffeull || ncheck > 0xfffffffeull) return CV_E_TOO_LARGE;
    // the ranges must be well formed for the kernel to stay inside the buffers
    if (!ranges_ok(tree_begin, ntrees, nnodes) || !ranges_ok(check_begin, ntrees, ncheck)) return CV_E_ARGS;
    return dispatch_one(ctx, ntrees, [&](Device &d, size_t, size_t, int) {   // tear-off batches are small
        CV_TRY(hipSetDevice(d.ordinal));
        Layout lay;
        const size_t o_kind = lay.take(nnodes), o_left = lay.take(4 * nnodes), o_right = lay.take(4 * nnodes);
        const size_t o_hash = lay.take(32 * nnodes), o_tb = lay.take(4 * (ntrees + 1)), o_root = lay.take(32 * ntrees);
        const size_t o_check = lay.take(32 * ncheck), o_cb = lay.take(4 * (ntrees + 1)), o_verdict = lay.take(ntrees);
        const size_t o_status = lay.take(ntrees), o_dig = lay.take(32 * nnodes), o_flag = lay.take(nnodes + 1);
        CV_TRY(d.pmt.ensure(lay.top));
        uint8_t *base = d.pmt.as<uint8_t>();
        hipStream_t s = d.stream;
        auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });
        if (nnodes) {
            CV_TRY(hipMemcpyAsync(base + o_kind, kind, nnodes, hipMemcpyHostToDevice, s));
            CV_TRY(hipMemcpyAsync(base + o_left, left, 4 * nnodes, hipMemcpyHostToDevice, s));
            CV_TRY(hipMemcpyAsync(base + o_right, right, 4 * nnodes, hipMemcpyHostToDevice, s));
            CV_TRY(hipMemcpyAsync(base + o_hash, leaf_hash, 32 * nnodes, hipMemcpyHostToDevice, s));
        }
        CV_TRY(hipMemcpyAsync(base + o_tb, tree_begin, 4 * (ntrees + 1), hipMemcpyHostToDevice, s));
        CV_TRY(hipMemcpyAsync(base + o_root, root, 32 * ntrees, hipMemcpyHostToDevice, s));
        if (ncheck) CV_TRY(hipMemcpyAsync(base + o_check, check, 32 * ncheck, hipMemcpyHostToDevice, s));
        CV_TRY(hipMemcpyAsync(base + o_cb, check_begin, 4 * (ntrees + 1), hipMemcpyHostToDevice, s));
        CV_TRY(cvk_pmt_verify((uint32_t)ntrees, base + o_kind, at<uint32_t>(base, o_left), at<uint32_t>(base, o_right),
                              base + o_hash, at<uint32_t>(base, o_tb), base + o_root, base + o_check,
                              at<uint32_t>(base, o_cb), at<uint32_t>(base, o_dig), base + o_flag, base + o_verdict,
                              base + o_status, s));
        CV_TRY(hipMemcpyAsync(verdict, base + o_verdict, ntrees, hipMemcpyDeviceToHost, s));
        if (status) CV_TRY(hipMemcpyAsync(status, base + o_status, ntrees, hipMemcpyDeviceToHost, s));
        CV_TRY(hipStreamSynchronize(s));
        drain.armed = false;
        return CV_OK;
    });
}

// ---------------------------------------------------------------- partial Merkle tree build (tear-offs)
// Entries of the level pyramid of a tree over L leaves and the most nodes a build over it emits: the pyramid plus
// one DuplicatedLeaf per level with an odd count above 1 (cv_pmt_build.h: cv_pmtb_pyramid_entries, cv_pmtb_bound).
static void pmtb_sizes(uint32_t L, uint64_t *pyramid, uint64_t *bound) {
    uint64_t p = 0, dup = 0;
    for (uint32_t n = L; n > 0; n = (n + 1) >> 1) {
        p += n;
        if (n == 1) break;
        dup += n & 1u;
    }
    *pyramid = p;
    *bound = p + dup;
}

uint64_t cv_partial_merkle_build_bound(size_t ntx, const uint32_t *tx_leaf_begin) {
    if (!tx_leaf_begin) return 0;
    uint64_t sum = 0;
    for (size_t t = 0; t < ntx; t++) {
        if (tx_leaf_begin[t + 1] < tx_leaf_begin[t]) continue;
        uint64_t p, b;
        pmtb_sizes(tx_leaf_begin[t + 1] - tx_leaf_begin[t], &p, &b);
        sum += b;
    }
    return sum;
}

namespace {
struct PmtbIn {
    size_t ntx;
    const uint32_t *txb;
    // explicit include lists over given leaf hashes ...
    const uint8_t *leaf_hash, *include;
    const uint32_t *inc_begin;
    // ... or leaf blobs and a keep mask (cv_filtered_build: keep != nullptr)
    const uint8_t *arena;
    uint64_t arena_bytes;
    const uint64_t *off;
    const uint32_t *len;
    const uint8_t *keep;
};
struct PmtbOut {
    size_t cap;
    uint8_t *kind;
    uint32_t *left, *right;
    uint8_t *node_hash;
    uint32_t *tree_begin;
    uint8_t *ids, *status;
    size_t *nnodes;
};
}  // namespace

// The checks both build calls share, all before any device work (a null context is the last of them): the leaf
// ranges well formed, the outputs present, the counts and the bound within 32 bits.  ws_off: each transaction's
// first pyramid entry (ntx + 1 entries, the last the total).
static int pmtb_check(cv_ctx *ctx, const PmtbIn &in, const PmtbOut &out, std::vector<uint32_t> *ws_off, uint64_t *bound) {
    if (in.ntx > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (!in.txb || !out.tree_begin || !out.status || !out.nnodes) return CV_E_ARGS;
    if (out.cap && (!out.kind || !out.left || !out.right || !out.node_hash)) return CV_E_ARGS;
    if (!ranges_ok(in.txb, in.ntx)) return CV_E_ARGS;
    const size_t nl = in.txb[in.ntx];
    if (in.keep ? (nl && (!in.off || !in.len)) : (nl && !in.leaf_hash)) return CV_E_ARGS;
    size_t ninc = 0;
    if (!in.keep) {
        if (!in.inc_begin || !ranges_ok(in.inc_begin, in.ntx)) return CV_E_ARGS;
        ninc = in.inc_begin[in.ntx];
        if (ninc && !in.include) return CV_E_ARGS;
    }
    if (nl > 0xfffffffeull || ninc > 0xfffffffeull) return CV_E_TOO_LARGE;
    uint64_t pyr = 0, bnd = 0;
    ws_off->assign(in.ntx + 1, 0);
    for (size_t t = 0; t < in.ntx; t++) {
        uint64_t p, b;
        pmtb_sizes(in.txb[t + 1] - in.txb[t], &p, &b);
        (*ws_off)[t] = (uint32_t)pyr;      // below 2^32 whenever the bound check passes
        pyr += p;
        bnd += b;
        if (bnd > 0xfffffffeull) return CV_E_TOO_LARGE;
    }
    (*ws_off)[in.ntx] = (uint32_t)pyr;
    *bound = bnd;
    if (!ctx) return CV_E_ARGS;
    return CV_OK;
}

// One device, the least loaded (tear-off batches are small), everything in d.pmt:
//   inputs (leaf hashes | the Merkle stage of the leaf blobs + their digests) | ranges | include lists or keep mask |
//   pyramid offsets | pyramid (dig, flag, size, pos) | counts | tree_begin | ids | status | node arrays (the bound)
// Two synchronisations: tree_begin, ids and status come back first, then — the total known and within nodes_cap —
// the node arrays' used part.
static int pmtb_run(cv_ctx *ctx, const PmtbIn &in, const PmtbOut &out, const std::vector<uint32_t> &ws_off, uint64_t bound) {
    return dispatch_one(ctx, in.ntx, [&](Device &d, size_t, size_t, int threads) {
        CV_TRY(hipSetDevice(d.ordinal));
        const size_t ntx = in.ntx, nl = in.txb[ntx], ninc = in.keep ? 0 : in.inc_begin[ntx];
        const size_t P = ws_off[ntx], B = (size_t)bound;
        MStage st;
        std::vector<uint8_t> packed;
        if (in.keep) {
            WorkerPool *pool = &d.workers(threads);
            st = mstage_plan(0, ntx, in.txb, in.off, in.len, pool);
            if (!mstage_in_bounds(st, in.arena_bytes)) return CV_E_ARGS;   // past the arena, or a leaf's off + len wraps
        }
        Layout lay;
        const size_t o_in = lay.take(in.keep ? st.total : 32 * nl), o_ldig = lay.take(in.keep ? 32 * nl + 32 : 0);
        const size_t o_txb = lay.take(4 * (ntx + 1)), o_inc = lay.take(32 * ninc), o_ib = lay.take(4 * (ntx + 1));
        const size_t o_keep = lay.take(in.keep ? nl : 0), o_wso = lay.take(4 * (ntx + 1)), o_dig = lay.take(32 * P);
        const size_t o_flag = lay.take(P), o_size = lay.take(4 * P), o_pos = lay.take(4 * P), o_cnt = lay.take(4 * ntx);
        const size_t o_tb = lay.take(4 * (ntx + 1)), o_ids = lay.take(32 * ntx), o_st = lay.take(ntx), o_kind = lay.take(B);
        const size_t o_left = lay.take(4 * B), o_right = lay.take(4 * B), o_hash = lay.take(32 * B);
        CV_TRY(d.pmt.ensure(lay.top + 16));
        uint8_t *base = d.pmt.as<uint8_t>();
        hipStream_t s = d.stream;
        auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });
        CvkPmtBuild a{};
        if (in.keep) {
            uint8_t *dv = base + o_in;
            if (st.compact) {
                packed.resize(st.total);
                mstage_pack(st, packed.data(), in.txb, in.arena, in.off, in.len, nullptr);
                CV_TRY(hipMemcpyAsync(dv, packed.data(), st.total, hipMemcpyHostToDevice, s));
            } else {
                CV_TRY(mstage_dma_direct(st, dv, in.txb, in.arena, in.off, in.len, s));
            }
            if (nl) CV_TRY(hipMemcpyAsync(base + o_keep, in.keep, nl, hipMemcpyHostToDevice, s));
            // the leaf kernel alone (no transactions: the tree sweep that follows keeps the levels)
            a.leaf_dig = at<uint32_t>(base, o_ldig);
            a.tx_leaf_begin = at<uint32_t>(dv, st.o_txb);
            CV_TRY(cvk_merkle(0, (uint32_t)nl, 0, dv + st.o_ar - st.lo, at<uint64_t>(dv, st.o_off),
                              at<uint32_t>(dv, st.o_len), a.tx_leaf_begin, at<uint32_t>(base, o_ldig), nullptr, nullptr, s));
            a.keep = base + o_keep;
        } else {
            if (nl) CV_TRY(hipMemcpyAsync(base + o_in, in.leaf_hash, 32 * nl, hipMemcpyHostToDevice, s));
            CV_TRY(hipMemcpyAsync(base + o_txb, in.txb, 4 * (ntx + 1), hipMemcpyHostToDevice, s));
            if (ninc) CV_TRY(hipMemcpyAsync(base + o_inc, in.include, 32 * ninc, hipMemcpyHostToDevice, s));
            CV_TRY(hipMemcpyAsync(base + o_ib, in.inc_begin, 4 * (ntx + 1), hipMemcpyHostToDevice, s));
            a.leaf_hash = base + o_in;
            a.tx_leaf_begin = at<uint32_t>(base, o_txb);
            a.include = base + o_inc;
            a.include_begin = at<uint32_t>(base, o_ib);
        }
        CV_TRY(hipMemcpyAsync(base + o_wso, ws_off.data(), 4 * (ntx + 1), hipMemcpyHostToDevice, s));
        a.ws_off = at<uint32_t>(base, o_wso);
        a.dig = at<uint32_t>(base, o_dig);
        a.flag = base + o_flag;
        a.size = at<uint32_t>(base, o_size);
        a.pos = at<uint32_t>(base, o_pos);
        a.count = at<uint32_t>(base, o_cnt);
        a.ids = base + o_ids;
        a.status = base + o_st;
        a.tree_begin = at<uint32_t>(base, o_tb);
        a.kind = base + o_kind;
        a.left = at<uint32_t>(base, o_left);
        a.right = at<uint32_t>(base, o_right);
        a.node_hash = base + o_hash;
        CV_TRY(cvk_pmt_build((uint32_t)ntx, &a, s));
        CV_TRY(hipMemcpyAsync(out.tree_begin, base + o_tb, 4 * (ntx + 1), hipMemcpyDeviceToHost, s));
        CV_TRY(hipMemcpyAsync(out.status, base + o_st, ntx, hipMemcpyDeviceToHost, s));
        if (out.ids) CV_TRY(hipMemcpyAsync(out.ids, base + o_ids, 32 * ntx, hipMemcpyDeviceToHost, s));
        CV_TRY(hipStreamSynchronize(s));
        const size_t nn = out.tree_begin[ntx];
        *out.nnodes = nn;
        if (nn > out.cap) {
            drain.armed = false;
            return CV_E_ARGS;              // tree_begin, status, ids and *nnodes are written, the node arrays are not
        }
        if (nn) {
            CV_TRY(hipMemcpyAsync(out.kind, base + o_kind, nn, hipMemcpyDeviceToHost, s));
            CV_TRY(hipMemcpyAsync(out.left, base + o_left, 4 * nn, hipMemcpyDeviceToHost, s));
            CV_TRY(hipMemcpyAsync(out.right, base + o_right, 4 * nn, hipMemcpyDeviceToHost, s));
            CV_TRY(hipMemcpyAsync(out.node_hash, base + o_hash, 32 * nn, hipMemcpyDeviceToHost, s));
            CV_TRY(hipStreamSynchronize(s));
        }
        drain.armed = false;
        return CV_OK;
    });
}

int cv_partial_merkle_build(cv_ctx *ctx, size_t ntx, const uint8_t *leaf_hash, const uint32_t *tx_leaf_begin,
                            const uint8_t *include, const uint32_t *include_begin, size_t nodes_cap, uint8_t *kind,
                            uint32_t *left, uint32_t *right, uint8_t *node_hash, uint32_t *tree_begin, uint8_t *ids,
                            uint8_t *status, size_t *nnodes) {
    if (ntx == 0) return CV_OK;
    const PmtbIn in{ntx, tx_leaf_begin, leaf_hash, include, include_begin, nullptr, 0, nullptr, nullptr, nullptr};
    const PmtbOut out{nodes_cap, kind, left, right, node_hash, tree_begin, ids, status, nnodes};
    std::vector<uint32_t> ws_off;
    uint64_t bound = 0;
    const int rc = pmtb_check(ctx, in, out, &ws_off, &bound);
    return rc != CV_OK ? rc : pmtb_run(ctx, in, out, ws_off, bound);
}

int cv_filtered_build(cv_ctx *ctx, size_t ntx, const uint8_t *leaf_arena, uint64_t leaf_arena_bytes,
                      const uint64_t *leaf_off, const uint32_t *leaf_len, const uint32_t *tx_leaf_begin,
                      const uint8_t *keep, size_t nodes_cap, uint8_t *kind, uint32_t *left, uint32_t *right,
                      uint8_t *node_hash, uint32_t *tree_begin, uint8_t *ids, uint8_t *status, size_t *nnodes) {
    if (ntx == 0) return CV_OK;
    if (!keep) return CV_E_ARGS;
    const PmtbIn in{ntx, tx_leaf_begin, nullptr, nullptr, nullptr, leaf_arena, leaf_arena_bytes, leaf_off, leaf_len, keep};
    const PmtbOut out{nodes_cap, kind, left, right, node_hash, tree_begin, ids, status, nnodes};
    std::vector<uint32_t> ws_off;
    uint64_t bound = 0;
    const int rc = pmtb_check(ctx, in, out, &ws_off, &bound);
    return rc != CV_OK ? rc : pmtb_run(ctx, in, out, ws_off, bound);
}

}  // extern "C"
