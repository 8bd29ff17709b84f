// hotkeys_san.cpp — TEST INFRASTRUCTURE: a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer over the
// hot-key route's steps (cv_hotkeys.h through tests/hotkeys_harness.cpp): the dedupe, tally, classify, the compactions,
// the classes and hot key rows, the gather and the merge.  It builds batches with keys out of its own generator — one
// record; all one key; all distinct; a pool of nine at 63, 64, 65, 127, 128 and 129 records; keys with hot_min - 1,
// hot_min and hot_min + 1 occurrences; more candidates than the capacity; 2,500 records past two blocks of the
// compaction — and checks the classes, perm, the counts, the merged bitmap (tail bits zero) and the status bytes
// against a std::map restatement, in all lane orders, with and without the tally's wave election, under hot_min 1, 2,
// 8 and n + 1.  The output arrays are sized exactly, so a write past them lands outside the allocation.
// tests/test_hotkeys_cpu.py compiles it with -fsanitize=address,undefined and runs it; exit status 0 and "ok" on success.
#include <array>
#include <cstdio>
#include <map>
#include <string>

#include "hotkeys_harness.cpp"

namespace {

typedef std::array<uint8_t, 32> Key;
typedef std::vector<Key> Rows;

uint64_t g_rng = 0x0123456789abcdefull;
uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_rng >> 33) % n);
}
Key fresh() {
    Key k;
    for (auto &b : k) b = (uint8_t)rnd(256);
    return k;
}
Rows pool(uint32_t k) {
    Rows p(k);
    for (auto &x : p) x = fresh();
    return p;
}
Rows draw(const Rows &p, uint32_t n) {
    Rows r(n);
    for (auto &x : r) x = p[rnd((uint32_t)p.size())];
    return r;
}
Rows occurrences(const std::vector<uint32_t> &counts) {
    Rows r;
    for (uint32_t c : counts) {
        const Key k = fresh();
        for (uint32_t j = 0; j < c; j++) r.insert(r.begin() + rnd((uint32_t)r.size() + 1), k);
    }
    return r;
}

int check(const std::string &name, const Rows &rows, uint32_t hot_min, uint32_t hot_cap) {
    const uint32_t n = (uint32_t)rows.size(), words = (n + 63) / 64;
    std::vector<uint32_t> pk(8 * (size_t)n), sig(16 * (size_t)n), len(n);
    std::vector<uint64_t> off(n);
    std::memcpy(pk.data(), rows.data(), 32 * (size_t)n);
    for (auto &w : sig) w = rnd(0x7fffffffu);
    for (uint32_t i = 0; i < n; i++) off[i] = ((uint64_t)rnd(0x7fffffffu) << 20) + rnd(1000), len[i] = rnd(4000);
    // the restatement: first-seen numbering, counts, candidates, the first hot_cap of them, the stable partition
    std::map<Key, uint32_t> seen;
    std::vector<uint32_t> index(n), count;
    for (uint32_t i = 0; i < n; i++) {
        auto it = seen.find(rows[i]);
        if (it == seen.end()) {
            it = seen.emplace(rows[i], (uint32_t)count.size()).first;
            count.push_back(0);
        }
        index[i] = it->second;
        count[it->second]++;
    }
    const uint32_t nk = (uint32_t)count.size();
    std::vector<uint32_t> want_cls(n, CVH_COLD);
    uint32_t cands = 0, hotkeys = 0;
    for (uint32_t k = 0; k < nk; k++)
        if (count[k] >= hot_min) {
            if (cands < hot_cap) want_cls[k] = cands, hotkeys++;
            cands++;
        }
    uint32_t nhot = 0;
    for (uint32_t i = 0; i < n; i++) nhot += want_cls[index[i]] != CVH_COLD;
    std::vector<uint32_t> want_perm(n);
    std::vector<uint64_t> want_bm(words, 0);
    std::vector<uint8_t> want_st(n);
    for (uint32_t i = 0, h = 0, c = 0; i < n; i++) {
        want_perm[i] = want_cls[index[i]] != CVH_COLD ? h++ : nhot + c++;
        const uint32_t f = hhk_fake_row(pk.data() + 8 * (size_t)i, sig.data() + 16 * (size_t)i, off[i], len[i]);
        if (f & 1u) want_bm[i >> 6] |= 1ull << (i & 63u);
        want_st[i] = (uint8_t)(f >> 1);
    }
    for (int order = 0; order < 3; order++)
        for (int elect = 0; elect < 2; elect++)
            for (int with_status = 0; with_status < 2; with_status++) {
                std::vector<uint32_t> cls(n), hotnum(n), perm(n, 0xEEEEEEEEu), head(4), hot_keys(8 * (size_t)hotkeys);
                std::vector<uint64_t> bm(words, 0xEEEEEEEEEEEEEEEEull);
                std::vector<uint8_t> st(n, 0xEE);
                const int rc = hhk_run(n, pk.data(), sig.data(), off.data(), len.data(), hot_min, hot_cap, order, elect,
                                       0x9e3779b97f4a7c15ull, cls.data(), hotnum.data(), perm.data(), head.data(),
                                       hot_keys.data(), bm.data(), with_status ? st.data() : nullptr);
                bool ok = rc == 0 && head[0] == nk && head[1] == hotkeys && head[2] == 1 && head[3] == nhot &&
                          cls == want_cls && perm == want_perm && bm == want_bm && (!with_status || st == want_st);
                for (uint32_t k = 0; ok && k < nk; k++)
                    if (want_cls[k] != CVH_COLD)
                        for (uint32_t i = 0; i < n; i++)
                            if (index[i] == k) {
                                ok = std::memcmp(hot_keys.data() + 8 * (size_t)want_cls[k], rows[i].data(), 32) == 0;
                                break;
                            }
                if (!ok) {
                    fprintf(stderr, "hotkeys_san: %s differs (n %u, hot_min %u, cap %u, order %d, elect %d, rc %d)\n",
                            name.c_str(), n, hot_min, hot_cap, order, elect, rc);
                    return 1;
                }
            }
    return 0;
}

int check_mins(const std::string &name, const Rows &rows) {
    int bad = 0;
    for (uint32_t hm : {1u, 2u, 8u, (uint32_t)rows.size() + 1}) bad |= check(name, rows, hm, 16384);
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    bad |= check_mins("n1", pool(1));
    bad |= check_mins("all_equal", Rows(300, fresh()));
    bad |= check_mins("all_distinct", pool(300));
    for (uint32_t n : {63u, 64u, 65u, 127u, 128u, 129u}) bad |= check_mins("n" + std::to_string(n), draw(pool(9), n));
    for (uint32_t hm : {2u, 3u, 8u}) bad |= check("around_min", occurrences({hm - 1, hm, hm + 1, 1, 1, 1}), hm, 16384);
    bad |= check("more_candidates_than_cap", occurrences({3, 1, 4, 2, 5, 1, 2, 6, 2, 3, 1, 2}), 2, 4);
    bad |= check("cap_1", occurrences({2, 2, 2, 1}), 2, 1);
    bad |= check_mins("past_two_blocks", draw(pool(700), 2500));
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
