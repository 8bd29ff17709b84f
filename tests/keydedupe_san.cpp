// keydedupe_san.cpp — TEST INFRASTRUCTURE: a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer over
// the device key dedupe (cv_keydedupe.h through tests/keydedupe_harness.cpp): insert, mark, the compaction and emit.
// It builds the cases of tests/keydedupe_cases.py itself, with keys out of its own generator — n = 1 and 2, equal and
// different; 63, 64 and 65 rows; all equal; all distinct; two keys alternating; keys that differ in byte 31 alone and
// in byte 0 alone; a first occurrence at the last index; an only repeat at the last index; 5,000 rows from a pool of
// four; keys of the 0xff.. kind (no points) repeated; 2,500 rows past two blocks of the compaction — and checks keys,
// key_index and nkeys against a std::map keyed by the 32 bytes, in all lane orders, with tables of the library's size
// and of the next power of two >= n (full or nearly so: probes chain and wrap) under several seeds.  Every array is
// sized exactly, so a read or write past it lands outside the allocation.  tests/test_keydedupe_cpu.py compiles it
// with -fsanitize=address,undefined and runs it; exit status 0 and "ok" on success.
#include <array>
#include <cstdio>
#include <map>
#include <string>

#include "keydedupe_harness.cpp"

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
Rows variants(int byte, uint32_t k, uint32_t n) {
    Rows p(k, fresh());
    for (uint32_t j = 0; j < k; j++) p[j][byte] = (uint8_t)(p[j][byte] + 1 + j);
    return draw(p, n);
}

int check(const std::string &name, const Rows &rows) {
    const uint32_t n = (uint32_t)rows.size();
    std::map<Key, uint32_t> seen;
    std::vector<Key> want_keys;
    std::vector<uint32_t> want_index(n);
    for (uint32_t i = 0; i < n; i++) {
        auto it = seen.find(rows[i]);
        if (it == seen.end()) {
            it = seen.emplace(rows[i], (uint32_t)want_keys.size()).first;
            want_keys.push_back(rows[i]);
        }
        want_index[i] = it->second;
    }
    std::vector<uint32_t> pk(8 * (size_t)n);
    std::memcpy(pk.data(), rows.data(), 32 * (size_t)n);
    uint64_t small = 1;
    while (small < n) small <<= 1;
    const uint64_t seeds[3] = {1, 0x9e3779b97f4a7c15ull, 0xdeadbeefcafef00dull};
    for (uint64_t slots : {(uint64_t)0, small})
        for (uint64_t seed : seeds)
            for (int order = 0; order < 3; order++) {
                // keys sized to the distinct keys exactly: a row written past the count lands outside
                std::vector<uint32_t> keys(8 * want_keys.size()), index(n, 0xEEEEEEEEu);
                uint32_t nkeys = 0xEEEEEEEEu;
                int wrapped = 0;
                const int rc = hkd_run(n, pk.data(), seed, slots, order, keys.data(), index.data(), &nkeys, &wrapped);
                if (rc != 0 || nkeys != want_keys.size() || index != want_index ||
                    std::memcmp(keys.data(), want_keys.data(), 32 * want_keys.size()) != 0) {
                    fprintf(stderr, "keydedupe_san: %s differs (n %u, slots %llu, seed %llx, order %d, rc %d, nkeys %u)\n",
                            name.c_str(), n, (unsigned long long)slots, (unsigned long long)seed, order, rc, nkeys);
                    return 1;
                }
            }
    return 0;
}

}  // namespace

int main() {
    int bad = 0;
    bad |= check("n1", pool(1));
    bad |= check("n2_equal", Rows(2, fresh()));
    bad |= check("n2_different", pool(2));
    for (uint32_t n : {63u, 64u, 65u}) bad |= check("n" + std::to_string(n), draw(pool(9), n));
    bad |= check("all_equal", Rows(300, fresh()));
    bad |= check("all_distinct", pool(300));
    bad |= check("all_distinct_full_table", pool(256));
    {
        const Rows p = pool(2);
        Rows r(301);
        for (uint32_t i = 0; i < 301; i++) r[i] = p[i % 2];
        bad |= check("alternating", r);
    }
    bad |= check("differ_in_byte_31", variants(31, 5, 200));
    bad |= check("differ_in_byte_0", variants(0, 5, 200));
    {
        Rows r = draw(pool(6), 130);
        r.push_back(fresh());
        bad |= check("first_occurrence_at_the_last_index", r);
    }
    {
        Rows r = draw(pool(6), 130);
        r[17] = fresh();
        r.push_back(r[17]);
        bad |= check("only_repeat_at_the_last_index", r);
    }
    {
        const Rows p = pool(4);
        Rows r(5000);
        for (uint32_t i = 0; i < 5000; i++) r[i] = p[(i * 7 / 3) % 4];
        bad |= check("signed_pool_of_4", r);
    }
    {
        Rows p(3);
        for (uint32_t j = 0; j < 3; j++) {
            p[j].fill(0xff);
            p[j][0] = (uint8_t)(0xf0 + j);
        }
        bad |= check("bad_keys_repeated", draw(p, 40));
    }
    bad |= check("past_two_blocks", draw(pool(700), 2500));
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
