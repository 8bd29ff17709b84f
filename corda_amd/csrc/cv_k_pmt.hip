// cv_k_pmt.hip — partial Merkle tree BUILD (tear-offs, the prover side of f3): count, scan, emit (cv_pmt_build.h).
// Shared helpers and every kernel declaration: cv_kcommon.h; launcher: cv_kernels.hip (cvk_pmt_build).
#include "cv_kcommon.h"
#include "cv_pmt_build.h"

// One lane per transaction: level 0 of its pyramid from the leaf hashes (leaf_hash: bytes as the caller gave them,
// or leaf_dig: the leaf kernel's digest words; exactly one is non-null), then sweep 1.  ws_off[t] = the
// transaction's first pyramid entry.  Writes ids (the roots), status and the node counts.
__global__ __launch_bounds__(CV_BLOCK) void cv_pmt_count_kernel(
    uint32_t ntx, const uint8_t *__restrict__ leaf_hash, const uint32_t *__restrict__ leaf_dig,
    const uint32_t *__restrict__ tx_leaf_begin, const uint8_t *__restrict__ include,
    const uint32_t *__restrict__ include_begin, const uint8_t *__restrict__ keep, const uint32_t *__restrict__ ws_off,
    uint32_t *__restrict__ dig, uint8_t *__restrict__ flag, uint32_t *__restrict__ size, uint32_t *__restrict__ pos,
    uint8_t *__restrict__ ids, uint8_t *__restrict__ status, uint32_t *__restrict__ count) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t >= ntx) return;
    const uint32_t lb = tx_leaf_begin[t], L = tx_leaf_begin[t + 1] - lb;
    const size_t w = ws_off[t];
    uint32_t *d0 = dig + 8 * w;
    for (uint32_t i = 0; i < L; i++) {
        uint32_t o[8];
        if (leaf_hash) {
            cv_load_digest(o, leaf_hash + 32 * (size_t)(lb + i));
        } else {
#pragma unroll
            for (int q = 0; q < 8; q++) o[q] = leaf_dig[8 * (size_t)(lb + i) + q];
        }
#pragma unroll
        for (int q = 0; q < 8; q++) d0[8 * (size_t)i + q] = o[q];
    }
    uint32_t root[8], cnt;
    const uint32_t ib = keep ? 0u : include_begin[t], ie = keep ? 0u : include_begin[t + 1];
    const int st = cv_pmtb_count(L, d0, flag + w, size + w, pos + w, keep ? nullptr : include + 32 * (size_t)ib, ie - ib,
                                 keep ? keep + lb : nullptr, root, cnt);
    uint4 *o = reinterpret_cast<uint4 *>(ids + (size_t)t * 32);
    o[0] = make_uint4(cv_bswap32(root[0]), cv_bswap32(root[1]), cv_bswap32(root[2]), cv_bswap32(root[3]));
    o[1] = make_uint4(cv_bswap32(root[4]), cv_bswap32(root[5]), cv_bswap32(root[6]), cv_bswap32(root[7]));
    status[t] = (uint8_t)st;
    count[t] = cnt;
}

// tree_begin[0 .. n] = the exclusive sum of count[0 .. n): ONE workgroup walks the counts CV_BLOCK at a time (a wave
// scan, the four wave totals through LDS, the running total in a register every lane carries) — tear-off batches
// are far too small for a multi-pass scan to pay.  The sum fits 32 bits: the caller bounded it.
__global__ __launch_bounds__(CV_BLOCK) void cv_pmt_scan_kernel(uint32_t n, const uint32_t *__restrict__ count,
                                                               uint32_t *__restrict__ tree_begin) {
    __shared__ uint32_t wsum[CV_BLOCK / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += CV_BLOCK) {          // uniform over the workgroup
        const uint32_t i = base + t;
        const uint32_t own = i < n ? count[i] : 0u;
        uint32_t inc = own;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(inc, d, 64);
            if ((int)lane >= d) inc += y;
        }
        if (lane == 63u) wsum[wv] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < CV_BLOCK / 64; k++) {
            const uint32_t s = wsum[k];
            before += k < wv ? s : 0u;
            total += s;
        }
        if (i < n) tree_begin[i] = carry + before + inc - own;
        carry += total;
        __syncthreads();
    }
    if (t == 0) tree_begin[n] = carry;
}

// One lane per transaction: sweep 3 of the transactions whose build succeeded, into the records the scan gave them.
__global__ __launch_bounds__(CV_BLOCK) void cv_pmt_emit_kernel(
    uint32_t ntx, const uint32_t *__restrict__ tx_leaf_begin, const uint32_t *__restrict__ ws_off,
    const uint32_t *__restrict__ dig, const uint8_t *__restrict__ flag, const uint32_t *__restrict__ size,
    uint32_t *__restrict__ pos, const uint8_t *__restrict__ status, const uint32_t *__restrict__ tree_begin,
    uint8_t *__restrict__ kind, uint32_t *__restrict__ left, uint32_t *__restrict__ right,
    uint8_t *__restrict__ node_hash) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t >= ntx || status[t] != CV_PMTB_OK) return;
    const uint32_t L = tx_leaf_begin[t + 1] - tx_leaf_begin[t];
    const size_t w = ws_off[t];
    cv_pmtb_emit(L, dig + 8 * w, flag + w, size + w, pos + w, tree_begin[t], kind, left, right, node_hash);
}
