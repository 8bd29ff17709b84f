// cv_hotkeys.h — the hot-key route: a batch of signatures split ON THE DEVICE by how often each key
// occurs.  Records of keys that occur at least hot_min times — the first hot_cap such keys in first-seen order — go
// through the keyed comb (cv_k_keyed.hip), the rest through the unkeyed path, and the verdicts come back in the
// caller's order.  The per-lane core of cv_k_hotkeys.hip; __host__ __device__, so tests/hotkeys_harness.cpp runs the
// lanes on the CPU one after another, in any order (the atomics reduce to plain operations there).
//
// The house rules of cv_keydedupe.h hold: a kernel per step, no lane reading what another lane of its kernel writes
// except through an atomic, no spin, flag or lock, every loop bounded.  Behind the dedupe (keys, key_index, nkeys):
//   tally    per record i: count[key_index[i]] grows by one — but only while it reads below hot_min (count zeroed by a
//            memset before).  THE HOT/COLD DECISION IS EXACT ALL THE SAME: a lane adds at most its own record, so the
//            counter never exceeds the key's true count; a lane skips only after it READ hot_min or more, so if any
//            lane skipped the counter had already reached hot_min (and the true count is no smaller); if none skipped
//            every record was added and the counter IS the true count.  Either way (counter >= hot_min) equals
//            (true count >= hot_min).  In the kernel alone the lanes of a wave that carry one key_index elect their
//            lowest lane, which adds their number in one atomic (cv_k_hotkeys.hip): the same argument with "its own
//            records" for "its own record", so every key's class is the same with and without the election and the
//            CPU harness can run every lane through cvh_tally(.., 1).
//   classify per key k (every lane reads *nkeys from device memory): cand[k] = k < nkeys && count[k] >= hot_min; the
//            lanes from nkeys on write 0, so the compaction runs over n entries whatever nkeys is
//   count / scan  the dedupe's ordered compaction over cand: cand[k] becomes hotnum, the candidates before k
//   keys     per key k: class[k] = hotnum when k is a candidate and hotnum < hot_cap, else CVH_COLD; a hot key writes
//            hot_keys[hotnum] = keys[k]; lane 0 writes head = {nkeys, hot keys, probe-ok, .}
//   flag     per record i: rank[i] = class[key_index[i]] != CVH_COLD
//   count / scan  the same compaction over rank: rank[i] becomes the hot records before i, head[3] = the hot records
//   -- the host reads head | hot_keys back here: the route's ONE synchronisation (the record flags and their scan run
//      BEFORE it, so the count of hot records comes back in the same copy instead of a second one) --
//   gather   per record i: perm[i] = rank[i] when hot, nhot + (i - rank[i]) when cold — a STABLE partition, hot
//            records at [0, nhot), cold ones at [nhot, n) — and sig, off, len copied to row perm[i]; a cold record
//            also copies pk, a hot one writes hot_kidx = class[key_index[i]].  The message arena is not copied.
//   merge    per record i, behind the two verifies: the verdict bit and the status byte of row perm[i]
// FIRST-SEEN, NOT BY-COUNT: when more keys qualify than the pool holds, the first hot_cap of them in first-seen order
// are hot.  That needs no sort and makes the classes, like everything above, A FUNCTION OF THE INPUT BYTES ALONE: the
// dedupe's numbering is one (cv_keydedupe.h), the classes follow from exact comparisons and index-ordered prefix sums.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cv_keydedupe.h"

#define CVH_COLD 0xffffffffu       // class of a cold key
#define CVH_HOT_MIN_DEFAULT 8u     // hot_min == 0: the project's "eight signatures per distinct key"
// words of head, which lies directly before hot_keys: ONE copy brings back head and the hot key rows
#define CVH_HEAD_NKEYS 0           // the distinct keys (0 after a probe error of the dedupe)
#define CVH_HEAD_HOTKEYS 1         // the hot keys
#define CVH_HEAD_OK 2              // 1, or 0 after a probe error of the dedupe
#define CVH_HEAD_NHOT 3            // the hot records (the record scan's total)
#define CVH_HEAD_WORDS 4
#define CVH_STAT_CAND 0            // the candidates (the key scan's total)
#define CVH_STAT_WORDS 4

struct CvHot {
    uint32_t n, hot_min, hot_cap;
    const uint32_t *pk;            // n * 8   } the caller's records
    const uint32_t *sig;           // n * 16  }
    const uint64_t *off;           // n       }
    const uint32_t *len;           // n       }
    const uint32_t *keys, *key_index, *nkeys;   // the dedupe's results
    uint32_t *count, *cand, *cls;  // n each (per key; the host does not know nkeys when it sizes them)
    uint32_t *stat;                // CVH_STAT_WORDS
    uint32_t *head;                // CVH_HEAD_WORDS, hot_keys directly behind
    uint32_t *hot_keys;            // n * 8
    uint32_t *rank, *perm;         // n each (per record)
    uint32_t *g_pk, *g_sig;        // n * 8, n * 16: the gathered records, hot rows first
    uint64_t *g_off;               // n
    uint32_t *g_len, *g_kidx;      // n each
    const uint64_t *bm_hot, *bm_cold;   // the sub-batches' verdict bitmaps (each from its own bit 0)
    const uint8_t *sub_status;     // n: hot rows, then cold rows
};

// the distinct keys as every step sees them: none after a probe error
CV_HD uint32_t cvh_nkeys(const CvHot &H) {
    const uint32_t nk = *H.nkeys;
    return nk <= H.n ? nk : 0u;
}

// w records of key k (w = 1 per lane; the kernel's wave leader passes its wave's number of them)
CV_HD void cvh_tally(const CvHot &H, uint32_t k, uint32_t w) {
    if (cvd_atomic_load(H.count + k) < H.hot_min) cvu_atomic_add(H.count + k, w);
}

CV_HD void cvh_classify(const CvHot &H, uint32_t k) { H.cand[k] = k < cvh_nkeys(H) && H.count[k] >= H.hot_min; }

// behind the scan of cand: cand[k] = the candidates before k, stat[CVH_STAT_CAND] = all of them
CV_HD void cvh_keys(const CvHot &H, uint32_t k) {
    const uint32_t nk = cvh_nkeys(H), num = H.cand[k];
    const bool hot = k < nk && H.count[k] >= H.hot_min && num < H.hot_cap;
    H.cls[k] = hot ? num : CVH_COLD;
    if (hot) cvu_copy8_aligned(H.hot_keys + 8 * (size_t)num, H.keys + 8 * (size_t)k);
    if (k == 0) {
        const uint32_t c = H.stat[CVH_STAT_CAND];
        H.head[CVH_HEAD_NKEYS] = nk;
        H.head[CVH_HEAD_HOTKEYS] = c < H.hot_cap ? c : H.hot_cap;
        H.head[CVH_HEAD_OK] = *H.nkeys <= H.n;
    }
}

CV_HD void cvh_flag(const CvHot &H, uint32_t i) { H.rank[i] = H.cls[H.key_index[i]] != CVH_COLD; }

// 16-byte rows between 16-byte aligned places
CV_HD void cvh_copy16(uint32_t *d, const uint32_t *s, int rows) {
#ifdef __HIP_DEVICE_COMPILE__
    uint4 *dv = reinterpret_cast<uint4 *>(d);
    const uint4 *sv = reinterpret_cast<const uint4 *>(s);
#pragma unroll
    for (int q = 0; q < rows; q++) dv[q] = sv[q];
#else
    for (int q = 0; q < 4 * rows; q++) d[q] = s[q];
#endif
}

// behind the scan of rank: rank[i] = the hot records before i, head[CVH_HEAD_NHOT] = all of them
CV_HD void cvh_gather(const CvHot &H, uint32_t i) {
    const uint32_t c = H.cls[H.key_index[i]], r = H.rank[i], nhot = H.head[CVH_HEAD_NHOT];
    const bool hot = c != CVH_COLD;
    const uint32_t p = hot ? r : nhot + (i - r);
    if (p >= H.n) return;                      // cannot happen: r < nhot for a hot record, i - r < n - nhot for a cold one
    H.perm[i] = p;
    cvh_copy16(H.g_sig + 16 * (size_t)p, H.sig + 16 * (size_t)i, 4);
    H.g_off[p] = H.off[i];
    H.g_len[p] = H.len[i];
    if (hot) H.g_kidx[p] = c;
    else cvh_copy16(H.g_pk + 8 * (size_t)p, H.pk + 8 * (size_t)i, 2);
}

// record i's verdict bit out of its sub-batch's bitmap; its status byte where the caller wants them
CV_HD uint32_t cvh_merge(const CvHot &H, uint32_t i, uint8_t *status) {
    const uint32_t p = H.perm[i], nhot = H.head[CVH_HEAD_NHOT];
    if (status) status[i] = H.sub_status[p];
    const uint64_t *bm = p < nhot ? H.bm_hot : H.bm_cold;
    const uint32_t q = p < nhot ? p : p - nhot;
    return (uint32_t)(bm[q >> 6] >> (q & 63u)) & 1u;
}

// ---------------------------------------------------------------- host: the workspace
#ifndef __HIP_DEVICE_COMPILE__
// Offsets into the workspace, each piece 16-byte aligned: the dedupe's own workspace (cvd_layout; its block sums serve
// the two compactions here too, one after another on the stream) | its results | the per-key and per-record arrays |
// head with hot_keys directly behind | the gathered records | the sub-batches' outputs.  The sub-batches take the
// gathered arrays by offset: the cold one starts at row nhot, at byte 32 nhot of g_pk, 64 nhot of g_sig and 8 nhot of
// g_off — multiples of 16 and 8 from 16-byte aligned bases, the alignment the verify kernels need — 4 nhot of g_len
// and byte nhot of the status rows (no alignment needed); each sub-batch has a bitmap of its own from bit 0.
struct CvhLayout {
    CvdLayout D;
    uint64_t dedupe, keys, key_index, nkeys, count, cand, cls, stat, head, hot_keys, rank, perm, g_pk, g_sig, g_off, g_len,
        g_kidx, bm_hot, bm_cold, sub_status, bytes;
};
inline CvhLayout cvh_layout(uint64_t n) {
    uint64_t top = 0;
    auto take = [&top](uint64_t bytes) {
        const uint64_t at = top;
        top += (bytes + 15) & ~(uint64_t)15;
        return at;
    };
    CvhLayout L{};
    L.D = cvd_layout(n);
    L.dedupe = take(L.D.bytes);
    L.keys = take(32 * n), L.key_index = take(4 * n), L.nkeys = take(16);
    L.count = take(4 * n), L.cand = take(4 * n), L.cls = take(4 * n), L.stat = take(4 * CVH_STAT_WORDS);
    L.head = take(4 * CVH_HEAD_WORDS), L.hot_keys = take(32 * n);
    L.rank = take(4 * n), L.perm = take(4 * n);
    L.g_pk = take(32 * n), L.g_sig = take(64 * n), L.g_off = take(8 * n), L.g_len = take(4 * n), L.g_kidx = take(4 * n);
    const uint64_t words = (n + 63) / 64;
    L.bm_hot = take(8 * words), L.bm_cold = take(8 * words), L.sub_status = take(n);
    L.bytes = top;
    return L;
}
// the hot key rows a call reads back at the most: no more keys than n / hot_min can occur hot_min times
inline uint64_t cvh_rows(uint64_t n, uint32_t hot_min, uint32_t hot_cap) {
    const uint64_t r = n / (hot_min ? hot_min : 1u);
    return r < hot_cap ? r : hot_cap;
}
inline CvDedupe cvh_dedupe_args(uint64_t n, const void *pk, void *ws, uint64_t seed, const CvhLayout &L) {
    uint8_t *w = static_cast<uint8_t *>(ws);
    return cvd_args(n, pk, w + L.keys, w + L.key_index, w + L.nkeys, w + L.dedupe, seed, L.D);
}
inline CvHot cvh_args(uint64_t n, uint32_t hot_min, uint32_t hot_cap, const void *pk, const void *sig, const void *off,
                      const void *len, void *ws, const CvhLayout &L) {
    uint8_t *w = static_cast<uint8_t *>(ws);
    auto u32 = [w](uint64_t o) { return reinterpret_cast<uint32_t *>(w + o); };
    CvHot H{};
    H.n = (uint32_t)n, H.hot_min = hot_min ? hot_min : CVH_HOT_MIN_DEFAULT, H.hot_cap = hot_cap;
    H.pk = static_cast<const uint32_t *>(pk), H.sig = static_cast<const uint32_t *>(sig);
    H.off = static_cast<const uint64_t *>(off), H.len = static_cast<const uint32_t *>(len);
    H.keys = u32(L.keys), H.key_index = u32(L.key_index), H.nkeys = u32(L.nkeys);
    H.count = u32(L.count), H.cand = u32(L.cand), H.cls = u32(L.cls), H.stat = u32(L.stat);
    H.head = u32(L.head), H.hot_keys = u32(L.hot_keys), H.rank = u32(L.rank), H.perm = u32(L.perm);
    H.g_pk = u32(L.g_pk), H.g_sig = u32(L.g_sig), H.g_off = reinterpret_cast<uint64_t *>(w + L.g_off);
    H.g_len = u32(L.g_len), H.g_kidx = u32(L.g_kidx);
    H.bm_hot = reinterpret_cast<const uint64_t *>(w + L.bm_hot), H.bm_cold = reinterpret_cast<const uint64_t *>(w + L.bm_cold);
    H.sub_status = w + L.sub_status;
    return H;
}
#endif
