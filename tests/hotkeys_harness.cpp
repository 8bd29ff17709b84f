// hotkeys_harness.cpp — TEST INFRASTRUCTURE: the hot-key route's steps (corda_amd/csrc/cv_hotkeys.h: the per-lane core
// is __host__ __device__) on the CPU, for tests/test_hotkeys_cpu.py, which builds this file into
// tests/_build/libcvhotkeys.so, and for tests/hotkeys_san.cpp, which includes it.
//
// hhk_run runs what the library enqueues (cvk_dedupe, cvk_hotkeys_front, cvk_hotkeys_gather, the two verifies,
// cvk_hotkeys_merge) over ONE workspace laid out as the library lays it out (cvh_layout), each step's lanes one after
// another in the order `order` names — 0 ascending, 1 descending, 2 one fixed shuffle (tests/keydedupe_harness.cpp).
// elect != 0 runs the tally as the kernel's waves run it: per 64 consecutive records, one add per distinct key_index
// with the number of its records; the classes must not depend on it.  The two verifies are replaced by hhk_fake, a
// function of the bytes of a gathered row (its key, signature, offset and length), so the merged verdicts and status
// bytes equal that function of the caller's records only if the gather moved every row whole to its place.
// The compactions run block by block as keydedupe_harness.cpp's scan_levels does.
#include "keydedupe_harness.cpp"

#include "../corda_amd/csrc/cv_hotkeys.h"

namespace {

void scan_ptr(uint32_t *arr, size_t m, uint32_t *total) {
    std::vector<uint32_t> v(arr, arr + m);
    scan_levels(v, total);
    std::memcpy(arr, v.data(), 4 * m);
}

// the stand-in for a verify: bit 0 the verdict, bit 1 the status byte
uint32_t hhk_fake(const uint32_t *key, const uint32_t *sig, uint64_t off, uint32_t len) {
    uint64_t h = 5 * off + 7 * (uint64_t)len;
    for (uint32_t q = 0; q < 8; q++) h += (uint64_t)key[q] * (q + 1);
    for (uint32_t q = 0; q < 16; q++) h += (uint64_t)sig[q] * (3 * q + 2);
    h ^= h >> 17;
    return (uint32_t)h & 3u;
}

}  // namespace

extern "C" {

uint64_t hhk_workspace(uint64_t n) { return cvh_layout(n).bytes; }
uint64_t hhk_rows(uint64_t n, uint32_t hot_min, uint32_t hot_cap) { return cvh_rows(n, hot_min, hot_cap); }
uint32_t hhk_fake_row(const uint32_t *key, const uint32_t *sig, uint64_t off, uint32_t len) { return hhk_fake(key, sig, off, len); }

// the layout's offsets in CvhLayout's order (21 of them, the last the size), for the alignment checks
void hhk_layout(uint64_t n, uint64_t *out21) {
    const CvhLayout L = cvh_layout(n);
    const uint64_t v[21] = {L.dedupe, L.keys, L.key_index, L.nkeys, L.count, L.cand, L.cls, L.stat, L.head, L.hot_keys, L.rank,
                            L.perm, L.g_pk, L.g_sig, L.g_off, L.g_len, L.g_kidx, L.bm_hot, L.bm_cold, L.sub_status, L.bytes};
    std::memcpy(out21, v, sizeof v);
}

// 0, or -2 after a probe error.  Outputs: cls[n], hotnum[n] (per key; entries from nkeys on: COLD / the candidates),
// perm[n], head[4], hot_keys[8 * hot keys], bitmap[ceil(n / 64)], status[n] (null: none).
int hhk_run(uint32_t n, const uint32_t *pk, const uint32_t *sig, const uint64_t *off, const uint32_t *len, uint32_t hot_min,
            uint32_t hot_cap, int order, int elect, uint64_t seed, uint32_t *cls, uint32_t *hotnum, uint32_t *perm,
            uint32_t *head, uint32_t *hot_keys, uint64_t *bitmap, uint8_t *status) {
    if (n == 0) return -3;
    const CvhLayout L = cvh_layout(n);
    // 16-byte aligned, as the device workspace is; poisoned, as nothing is expected in it
    std::vector<uint64_t> block((L.bytes + 15) / 8 + 2, 0xEEEEEEEEEEEEEEEEull);
    uint8_t *ws = reinterpret_cast<uint8_t *>(block.data());
    ws += (16 - (reinterpret_cast<uintptr_t>(ws) & 15)) & 15;
    const CvDedupe D = cvh_dedupe_args(n, pk, ws, seed, L);
    const CvHot H = cvh_args(n, hot_min, hot_cap, pk, sig, off, len, ws, L);
    // cvk_dedupe
    std::memset(D.tab, 0xff, 4 * (D.mask + 1) + 4 * CVD_STAT_WORDS);
    for (uint32_t i : lanes(n, order)) cvd_insert(D, i);
    for (uint32_t i : lanes(n, order)) cvd_mark(D, i);
    scan_ptr(D.number, n, D.stat + CVD_STAT_TOTAL);
    for (uint32_t i : lanes(n, order)) cvd_emit(D, i);
    if (*D.nkeys == CVD_NONE) return -2;
    // cvk_hotkeys_front
    std::memset(H.count, 0, 4 * (size_t)n);
    if (elect) {
        for (uint32_t w0 = 0; w0 < n; w0 += 64) {
            const uint32_t w1 = w0 + 64 < n ? w0 + 64 : n;
            std::vector<bool> done(w1 - w0, false);
            for (uint32_t a = w0; a < w1; a++) {
                if (done[a - w0]) continue;
                uint32_t group = 0;
                for (uint32_t b = a; b < w1; b++)
                    if (H.key_index[b] == H.key_index[a]) done[b - w0] = true, group++;
                cvh_tally(H, H.key_index[a], group);
            }
        }
    } else {
        for (uint32_t i : lanes(n, order)) cvh_tally(H, H.key_index[i], 1);
    }
    for (uint32_t k : lanes(n, order)) cvh_classify(H, k);
    scan_ptr(H.cand, n, H.stat + CVH_STAT_CAND);
    for (uint32_t k : lanes(n, order)) cvh_keys(H, k);
    for (uint32_t i : lanes(n, order)) cvh_flag(H, i);
    scan_ptr(H.rank, n, H.head + CVH_HEAD_NHOT);
    // the read-back
    std::memcpy(head, H.head, 4 * CVH_HEAD_WORDS);
    if (head[CVH_HEAD_HOTKEYS]) std::memcpy(hot_keys, H.hot_keys, 32 * (size_t)head[CVH_HEAD_HOTKEYS]);
    std::memcpy(cls, H.cls, 4 * (size_t)n);
    std::memcpy(hotnum, H.cand, 4 * (size_t)n);
    const uint32_t nhot = head[CVH_HEAD_NHOT];
    // cvk_hotkeys_gather, the two "verifies" over their sub-batches, cvk_hotkeys_merge
    for (uint32_t i : lanes(n, order)) cvh_gather(H, i);
    std::memcpy(perm, H.perm, 4 * (size_t)n);
    uint64_t *bh = const_cast<uint64_t *>(H.bm_hot), *bc = const_cast<uint64_t *>(H.bm_cold);
    uint8_t *sub = const_cast<uint8_t *>(H.sub_status);
    for (uint32_t w = 0; w < (nhot + 63) / 64; w++) bh[w] = 0;
    for (uint32_t w = 0; w < (n - nhot + 63) / 64; w++) bc[w] = 0;
    for (uint32_t p = 0; p < n; p++) {
        const bool hot = p < nhot;
        const uint32_t *key = hot ? H.hot_keys + 8 * (size_t)H.g_kidx[p] : H.g_pk + 8 * (size_t)p;
        const uint32_t f = hhk_fake(key, H.g_sig + 16 * (size_t)p, H.g_off[p], H.g_len[p]);
        const uint32_t q = hot ? p : p - nhot;
        if (f & 1u) (hot ? bh : bc)[q >> 6] |= 1ull << (q & 63u);
        sub[p] = (uint8_t)(f >> 1);
    }
    // cv_hot_merge_kernel: a wave per word, the lanes past n contribute 0, a wave at or past n stores nothing
    for (uint32_t w0 = 0; w0 < n; w0 += 64) {
        uint64_t word = 0;
        for (uint32_t i : lanes(n - w0 < 64 ? n - w0 : 64, order))
            if (cvh_merge(H, w0 + i, status)) word |= 1ull << i;
        bitmap[w0 >> 6] = word;
    }
    return 0;
}

}  // extern "C"
