// uniq_snapshot_harness.cpp — TEST INFRASTRUCTURE: snapshot, clear and install of the uniqueness set (the per-lane
// pieces cvu_snap_occupied / cvu_snap_emit / cvu_snap_close of corda_amd/csrc/cv_uniq.h, and the load path against a
// fresh table) on the CPU, for tests/test_uniq_snapshot_cpu.py, which builds this file into
// tests/_build/libcvuniqsnap.so, and for tests/uniq_snapshot_san.cpp, which includes it.  It includes
// tests/uniq_harness.cpp unchanged for the set itself (HSet, huq_*).
//
// A SSet is a HSet with the epoch cv_uniq keeps (cv_host.h); hus_commit / hus_load / hus_reserve are huq_*'s with the
// epoch advanced as cv_api_uniq.cpp advances it.  hus_snapshot is cv_uniq_snapshot: the same cursor, window
// (max(2 * max_entries, 65,536) slots), record buffers of exactly min(max_entries, window) entries (a write past them
// lands outside the allocation) and the steps of cvk_uniq_snapshot — count and emit with the lanes of the whole grid
// (the lanes past the window included) ONE AFTER ANOTHER in the order `order` names, the scan between them serial.
// Return codes as the C-ABI's: 0, -1 (the device result out of range), -3, -5.
#include "uniq_harness.cpp"

namespace {

struct SSet {
    HSet *h;
    uint64_t epoch;
};

const uint64_t kDone = ~0ull;
const uint32_t kBlock = 256;          // CV_BLOCK: the grid is whole blocks

HSet *hs(void *p) { return static_cast<SSet *>(p)->h; }
void touch(void *p) {
    SSet *s = static_cast<SSet *>(p);
    if (++s->epoch == 0) s->epoch = 1;
}

}  // namespace

extern "C" {

void *hus_open(uint64_t capacity, uint64_t seed, uint64_t epoch) {
    return new SSet{static_cast<HSet *>(huq_open(capacity, seed)), epoch | 1};
}
void hus_close(void *p) {
    huq_close(hs(p));
    delete static_cast<SSet *>(p);
}
void *hus_set(void *p) { return hs(p); }          // for huq_stats and huq_lookup, which change nothing

int hus_commit(void *p, uint32_t ntx, const uint32_t *key, const uint32_t *begin, const uint32_t *id, const uint32_t *caller,
               const uint8_t *enable, int max_rounds, int order, uint8_t *tx_status, uint8_t *state_conflict,
               uint32_t *cons_id, uint32_t *cons_index, uint32_t *cons_caller) {
    if (ntx && hs(p)->resident + begin[ntx] <= hs(p)->capacity) touch(p);      // uniq_decide ran
    return huq_commit(hs(p), ntx, key, begin, id, caller, enable, max_rounds, order, tx_status, state_conflict, cons_id,
                      cons_index, cons_caller);
}
int hus_load(void *p, uint32_t n, const uint32_t *key, const uint32_t *id, uint32_t *index, const uint32_t *caller, int order) {
    if (n && hs(p)->resident + n <= hs(p)->capacity) touch(p);
    return huq_load(hs(p), n, key, id, index, caller, order);
}
int hus_reserve(void *p, uint64_t capacity, int order) {
    const uint32_t mask = hs(p)->T.mask;
    const int rc = huq_reserve(hs(p), capacity, order);
    if (hs(p)->T.mask != mask) touch(p);          // a rehash
    return rc;
}

int hus_snapshot(void *p, uint64_t cursor[2], uint64_t max_entries, int order, uint32_t *key, uint32_t *id, uint32_t *index,
                 uint32_t *caller, uint64_t *n) {
    SSet *s = static_cast<SSet *>(p);
    HSet *h = s->h;
    if (max_entries == 0 || !cursor || !n || !key || !id || !index || !caller) return -3;
    if (max_entries > (1ull << 30)) return -5;
    if (cursor[0] == kDone) {
        *n = 0;
        return 0;
    }
    const uint64_t slots = (uint64_t)h->T.mask + 1;
    if (cursor[0] == 0 ? cursor[1] != 0 : (cursor[1] != s->epoch || cursor[0] >= slots)) return -3;
    const uint64_t b = cursor[0], look = 2 * max_entries > 65536 ? 2 * max_entries : 65536;
    const uint64_t e = b + look < slots ? b + look : slots;
    const size_t m = (size_t)(max_entries < e - b ? max_entries : e - b);
    std::vector<uint32_t> okey(8 * m), oid(8 * m), oix(m), ocal(m), out(CVU_SNAP_WORDS, 0xdeadbeefu);
    CvUniqSnap S{};
    S.slot_begin = (uint32_t)b;
    S.slot_end = (uint32_t)e;
    S.max_entries = (uint32_t)max_entries;
    S.key = okey.data();
    S.id = oid.data();
    S.index = oix.data();
    S.caller = ocal.data();
    S.out = out.data();
    const size_t grid = (size_t)((e - b + kBlock - 1) / kBlock) * kBlock;
    const std::vector<uint32_t> gl = lanes(grid, order);
    std::vector<uint32_t> flag(grid), rank(grid);
    for (uint32_t i : gl) flag[i] = cvu_snap_occupied(h->T, S, i);             // count
    uint32_t run = 0;                                                          // scan
    for (size_t i = 0; i < grid; i++) {
        rank[i] = run;
        run += flag[i];
    }
    out[CVU_SNAP_TOTAL] = run;
    for (uint32_t i : gl) {                                                    // emit
        if (flag[i]) cvu_snap_emit(h->T, S, i, rank[i]);
        if (i == 0) cvu_snap_close(S);
    }
    const uint64_t cnt = out[CVU_SNAP_COUNT], next = out[CVU_SNAP_NEXT];
    if (cnt > m || next <= b || next > e) return -1;
    memcpy(key, okey.data(), 32 * cnt);
    memcpy(id, oid.data(), 32 * cnt);
    memcpy(index, oix.data(), 4 * cnt);
    memcpy(caller, ocal.data(), 4 * cnt);
    *n = cnt;
    cursor[0] = next == slots ? kDone : next;
    cursor[1] = s->epoch;
    return 0;
}

int hus_clear(void *p) {
    HSet *h = hs(p);
    touch(p);
    memset(h->T.occ, 0, 4 * ((size_t)h->T.mask + 1));
    h->resident = 0;
    return 0;
}

// cv_uniq_install: a fresh table of max(capacity, n) with `seed`, the load path against it, the swap on success
int hus_install(void *p, uint64_t n, const uint32_t *key, const uint32_t *id, uint32_t *index, const uint32_t *caller,
                uint64_t seed, int order) {
    HSet *h = hs(p);
    if (n == 0) return hus_clear(p);
    if (!key || !id || !index || !caller) return -3;
    if (n > (1ull << 30)) return -5;
    HSet fresh;
    fresh.capacity = h->capacity > n ? h->capacity : (size_t)n;
    carve(fresh.mem, fresh.capacity, seed, &fresh.T);
    const int rc = huq_load(&fresh, (uint32_t)n, key, id, index, caller, order);
    if (rc) return rc;                            // the old table is untouched
    h->mem.swap(fresh.mem);
    h->T = fresh.T;
    h->capacity = fresh.capacity;
    h->resident = (size_t)n;
    h->probe = fresh.probe;
    h->wraps += fresh.wraps;
    touch(p);
    return 0;
}

}  // extern "C"
