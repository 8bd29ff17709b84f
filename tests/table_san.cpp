// table_san.cpp — TEST INFRASTRUCTURE: a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer over
// the one probe walk and the one size function of corda_amd/csrc/cv_table.h, alone: every probe of the library's hash
// tables is cv_walk with a visitor, so this is where all of them can break at once.  The visitors touch an array of
// exactly mask + 1 words on the heap (a slot past it lands outside the allocation) and write down the slots they were
// given.  tests/test_table_cpu.py compiles it with -fsanitize=address,undefined and runs it; exit status 0 and "ok"
// on success.
#include <cstdio>
#include <vector>

#include "../corda_amd/csrc/cv_table.h"

namespace {

int g_bad = 0;
#define EXPECT(cond)                                                \
    do {                                                            \
        if (!(cond)) {                                              \
            printf("FAIL line %d: %s\n", __LINE__, #cond);          \
            g_bad++;                                                \
        }                                                           \
    } while (0)

// a walk over a table of mask + 1 words that stops at the stop_at-th slot it sees (0: never)
template <class I> struct Run {
    std::vector<uint32_t> seen;
    CvWalk<I> w;
    Run(I mask, I start, uint32_t *wraps, uint32_t stop_at) {
        std::vector<uint32_t> tab((size_t)mask + 1, 0);
        w = cv_walk(mask, start, wraps, [&](I slot) {
            tab[(size_t)slot]++;
            seen.push_back((uint32_t)slot);
            return (uint32_t)seen.size() == stop_at;
        });
        for (uint32_t c : tab) EXPECT(c <= 1);                     // no slot twice
    }
};

uint64_t slots_restated(uint64_t n, uint64_t floor) {
    for (int b = 0; b < 64; b++)
        if ((1ull << b) >= floor && (1ull << b) >= 2 * n) return 1ull << b;
    return 0;
}

}  // namespace

int main() {
    {   // from slot 15, stopping at the third slot: 15, 0, 1 and one wrap
        uint32_t wraps = 0;
        Run<uint32_t> r(15, 15, &wraps, 3);
        EXPECT(r.w.stopped && r.w.n == 3 && r.w.slot == 1 && wraps == 1);
        EXPECT(r.seen == (std::vector<uint32_t>{15, 0, 1}));
        const CvWalk<uint32_t> w = cv_walk(15u, 3u, &wraps, [](uint32_t slot) { return slot == 5 ? 7 : 0; });
        EXPECT(w.stopped == 7 && w.slot == 5 && w.n == 3 && wraps == 1);   // the visitor's own stop value, and where
    }
    for (uint32_t start : {0u, 7u, 15u}) {   // a visitor that stops at once: one slot, no wrap, also from slot 15
        uint32_t wraps = 0;
        Run<uint32_t> r(15, start, &wraps, 1);
        EXPECT(r.w.stopped && r.w.n == 1 && wraps == 0);
        EXPECT(r.seen == (std::vector<uint32_t>{start}));
    }
    for (uint32_t start : {0u, 5u, 15u}) {   // a visitor that never stops: each of the 16 slots once, one wrap
        uint32_t wraps = 0;
        Run<uint32_t> r(15, start, &wraps, 0);
        EXPECT(!r.w.stopped && r.w.n == 16 && r.seen.size() == 16 && wraps == 1);
        for (uint32_t j = 0; j < r.seen.size(); j++) EXPECT(r.seen[j] == ((start + j) & 15));
    }
    {   // the same with no wraps counter: nothing is written anywhere (a write through null is the sanitizer's find)
        Run<uint32_t> r(15, 9, nullptr, 0);
        EXPECT(!r.w.stopped && r.w.n == 16 && r.seen.size() == 16);
        Run<uint32_t> q(15, 15, nullptr, 3);
        EXPECT(q.w.stopped && q.w.n == 3);
    }
    {   // a start above the mask is reduced by it
        uint32_t wraps = 0;
        Run<uint32_t> r(15, 0xabcdef37u, &wraps, 2);
        EXPECT(r.w.stopped && r.w.n == 2 && wraps == 0);
        EXPECT(r.seen == (std::vector<uint32_t>{7, 8}));
    }
    for (uint32_t start : {0u, 1u}) {   // mask 1, the dedupe's floor: exactly two slots
        uint32_t wraps = 0;
        Run<uint32_t> r(1, start, &wraps, 0);
        EXPECT(!r.w.stopped && r.w.n == 2 && wraps == 1);
        EXPECT(r.seen == (std::vector<uint32_t>{start, 1 - start}));
    }
    {   // 64-bit slots, as the dedupe's table has them
        uint32_t wraps = 0;
        Run<uint64_t> r(15, 0xfedcba987654321full, &wraps, 0);
        EXPECT(!r.w.stopped && r.w.n == 16 && r.seen.size() == 16 && r.seen[0] == 15 && r.seen[1] == 0 && wraps == 1);
    }
    for (uint64_t floor : {2ull, 16ull})
        for (uint64_t n : {0ull, 1ull, 7ull, 8ull, 9ull, (1ull << 20) - 1, 1ull << 20, 1ull << 30}) {
            const uint64_t s = cv_table_slots(n, floor);
            EXPECT(s == slots_restated(n, floor));
            EXPECT((s & (s - 1)) == 0 && s >= floor && s >= 2 * n && (s == floor || s / 2 < 2 * n));
        }
    EXPECT(cv_table_slots(8, 16) == 16 && cv_table_slots(9, 16) == 32 && cv_table_slots(0, 2) == 2 &&
           cv_table_slots(1ull << 30, 16) == 1ull << 31);
    if (g_bad) return 1;
    printf("ok\n");
    return 0;
}
