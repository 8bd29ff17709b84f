// uniq_harness.cpp — TEST INFRASTRUCTURE: the uniqueness set's per-lane core (corda_amd/csrc/cv_uniq.h;
// __host__ __device__) on the CPU, for tests/test_uniq_cpu.py, which builds this file into tests/_build/libcvuniq.so,
// and for tests/uniq_san.cpp, which includes it.
//
// A HSet is what cv_uniq is in cv_api_uniq.cpp, in host memory; huq_commit / huq_load / huq_lookup / huq_reserve run the
// steps the launchers of cv_kernels.hip enqueue (cvk_uniq_front, _round, _finish, _load, _lookup, _rehash), each
// step's lanes ONE AFTER ANOTHER in the order `order` names: 0 ascending, 1 descending, 2 one fixed shuffle.  The
// results must not depend on it.  Return codes as the C-ABI's: 0, -2 (a probe ran out), -3, -4.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../corda_amd/csrc/cv_uniq.h"

namespace {

struct HSet {
    std::vector<uint32_t> mem;
    CvUniqTable T{};
    size_t capacity = 0, resident = 0;
    uint64_t rounds = 0, tail = 0, probe = 0, wraps = 0;
};

// a zeroed table for `capacity` states in mem: the library's size (cv_table.h) and carve-up (cv_uniq.h)
void carve(std::vector<uint32_t> &mem, size_t capacity, uint64_t seed, CvUniqTable *T) {
    const size_t slots = (size_t)cv_table_slots(capacity, 16);
    mem.assign(CVU_SLOT_BYTES * slots / 4, 0);
    *T = cvu_carve(mem.data(), slots, seed);
}

std::vector<uint32_t> lanes(size_t n, int order) {
    std::vector<uint32_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (uint32_t)(order == 1 ? n - 1 - i : i);
    if (order == 2) {
        uint64_t x = 0x9e3779b97f4a7c15ull;
        for (size_t i = n; i > 1; i--) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(v[i - 1], v[(size_t)((x >> 33) % i)]);
        }
    }
    return v;
}

int fold(HSet *h, const uint32_t *dstat) {
    h->probe = dstat[CVU_D_MAXPROBE];
    h->wraps += dstat[CVU_D_WRAPS];
    return dstat[CVU_D_ERROR] ? -2 : 0;
}

}  // namespace

extern "C" {

void *huq_open(uint64_t capacity, uint64_t seed) {
    HSet *h = new HSet();
    h->capacity = capacity ? capacity : 1;
    carve(h->mem, h->capacity, seed, &h->T);
    return h;
}

void huq_close(void *p) { delete static_cast<HSet *>(p); }

void huq_stats(void *p, uint64_t out[7]) {
    HSet *h = static_cast<HSet *>(p);
    const uint64_t v[7] = {h->resident, h->capacity, (uint64_t)h->T.mask + 1, h->rounds, h->tail, h->probe, h->wraps};
    memcpy(out, v, sizeof v);
}

int huq_reserve(void *p, uint64_t capacity, int order) {
    HSet *h = static_cast<HSet *>(p);
    if (capacity <= h->capacity) return 0;
    if (cv_table_slots(capacity, 16) == (uint64_t)h->T.mask + 1) {
        h->capacity = capacity;
        return 0;
    }
    std::vector<uint32_t> mem;
    CvUniqTable to{};
    carve(mem, capacity, h->T.seed, &to);
    uint32_t dstat[CVU_D_WORDS] = {};
    for (uint32_t s : lanes((size_t)h->T.mask + 1, order)) cvu_rehash(h->T, to, s, dstat);
    const int rc = fold(h, dstat);
    if (rc) return rc;
    h->mem.swap(mem);
    h->T = to;
    h->capacity = capacity;
    return 0;
}

int huq_commit(void *p, uint32_t ntx, const uint32_t *key, const uint32_t *begin, const uint32_t *id, const uint32_t *caller,
               const uint8_t *enable, int max_rounds, int order, uint8_t *tx_status, uint8_t *state_conflict,
               uint32_t *cons_id, uint32_t *cons_index, uint32_t *cons_caller) {
    HSet *h = static_cast<HSet *>(p);
    if (ntx == 0) return 0;
    const uint32_t S = begin[ntx];
    if (h->resident + S > h->capacity) return -4;
    std::vector<uint32_t> btab((size_t)cv_table_slots(S, 16), CVU_NONE), rep(S + 1), res(S + 1), stx(S + 1), owner(S + 1), last(S + 1);
    std::vector<uint32_t> s0(ntx), s1(ntx), dstat(CVU_D_WORDS, 0);
    CvUniqBatch B{};
    B.ntx = ntx;
    B.nstates = S;
    B.key = key;
    B.begin = begin;
    B.id = id;
    B.caller = caller;
    B.enable = enable;
    B.btab = btab.data();
    B.bmask = (uint32_t)(btab.size() - 1);
    B.rep = rep.data();
    B.res = res.data();
    B.state_tx = stx.data();
    B.owner = owner.data();
    B.last = last.data();
    B.tx_status = tx_status;
    B.state_conflict = state_conflict;
    B.cons_id = cons_id;
    B.cons_index = cons_index;
    B.cons_caller = cons_caller;
    B.dstat = dstat.data();
    memset(cons_id, 0, 32 * (size_t)S);
    memset(cons_index, 0, 4 * (size_t)S);
    memset(cons_caller, 0, 4 * (size_t)S);
    uint32_t *cur = s0.data(), *nxt = s1.data();
    const std::vector<uint32_t> tl = lanes(ntx, order), sl = lanes(S, order);
    // cvk_uniq_front
    for (uint32_t t : tl) cvu_init(B, cur, t);
    for (uint32_t i : sl) cvu_group(h->T, B, cur, i);
    // cvk_uniq_round while a request is undecided
    uint64_t rounds = 0;
    bool undecided = true;
    while (undecided && rounds < (uint64_t)max_rounds) {
        owner.assign(owner.size(), CVU_NONE);
        for (uint32_t t : tl) cvu_claim(B, cur, t);
        for (uint32_t t : tl) dstat[CVU_D_ROUND0 + rounds] += cvu_decide(B, cur, nxt, t);
        std::swap(cur, nxt);
        undecided = dstat[CVU_D_ROUND0 + rounds] != 0;
        rounds++;
    }
    // cvk_uniq_finish
    owner.assign(owner.size(), CVU_NONE);
    for (uint32_t t : tl) cvu_own(B, cur, t);
    if (undecided)
        for (uint32_t t = 0; t < ntx; t++)
            if (cur[t] == CVU_UNDECIDED) cvu_tail_one(B, cur, t);
    for (uint32_t t : tl) dstat[CVU_D_INSERTED] += cvu_report(h->T, B, cur, t);
    h->resident += dstat[CVU_D_INSERTED];
    h->rounds = rounds;
    h->tail = dstat[CVU_D_TAIL];
    return fold(h, dstat.data());
}

int huq_lookup(void *p, uint32_t n, const uint32_t *key, int order, uint8_t *found, uint32_t *cons_id, uint32_t *cons_index,
               uint32_t *cons_caller) {
    HSet *h = static_cast<HSet *>(p);
    uint32_t dstat[CVU_D_WORDS] = {};
    memset(cons_id, 0, 32 * (size_t)n);
    memset(cons_index, 0, 4 * (size_t)n);
    memset(cons_caller, 0, 4 * (size_t)n);
    for (uint32_t i : lanes(n, order)) cvu_lookup(h->T, key, i, found, cons_id, cons_index, cons_caller, dstat);
    return fold(h, dstat);
}

int huq_load(void *p, uint32_t n, const uint32_t *key, const uint32_t *id, uint32_t *index, const uint32_t *caller, int order) {
    HSet *h = static_cast<HSet *>(p);
    if (n == 0) return 0;
    if (h->resident + n > h->capacity) return -4;
    std::vector<uint32_t> btab((size_t)cv_table_slots(n, 16), CVU_NONE), rep(n), res(n), dstat(CVU_D_WORDS, 0);
    CvUniqBatch B{};
    B.nstates = n;
    B.key = key;
    B.id = id;
    B.cons_index = index;
    B.caller = caller;
    B.btab = btab.data();
    B.bmask = (uint32_t)(btab.size() - 1);
    B.rep = rep.data();
    B.res = res.data();
    B.dstat = dstat.data();
    const std::vector<uint32_t> sl = lanes(n, order);
    for (uint32_t i : sl) cvu_group(h->T, B, nullptr, i);
    for (uint32_t i : sl) cvu_load_check(B, i);
    if (dstat[CVU_D_ERROR]) return -2;
    if (dstat[CVU_D_BAD]) return -3;
    for (uint32_t i : sl) cvu_load_put(h->T, B, i);
    const int rc = fold(h, dstat.data());
    if (rc == 0) h->resident += n;
    return rc;
}

}  // extern "C"
