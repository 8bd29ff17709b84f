// uniq_snapshot_san.cpp — TEST INFRASTRUCTURE: a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer
// over snapshot, clear and install of the uniqueness set (cv_uniq.h through tests/uniq_snapshot_harness.cpp).  It
// generates its cases itself and checks them against a std::map, in all three lane orders:
//   wrap     16-slot tables filled to their capacity of 8 under seeds 0..63 (some of whose probes pass the last slot),
//            snapshotted whole and one, seven, eight and nine records a call
//   seams    3,000 entries in 8,192 slots, whole and in chunks of 7, 64, 65, 256, 257 and 1,000 records: the chunks
//            concatenated are the whole pass byte for byte; 300 entries one record a call
//   install  the snapshot into a set of another seed and a smaller capacity: every key looked up; a repeated key
//            leaves the set as it was; clear; the epoch refuses a pass continued after each of them
// The harness sizes the record buffers of a call exactly, and the buffers here are sized to max_entries, so a write
// past either lands outside an allocation.  tests/test_uniq_snapshot_cpu.py compiles it with
// -fsanitize=address,undefined and runs it; exit status 0 and "ok" on success.
#include <array>
#include <cstdio>
#include <map>

#include "uniq_snapshot_harness.cpp"

namespace {

typedef std::array<uint32_t, 8> Key;
struct Rec {
    Key id;
    uint32_t index, caller;
    bool operator==(const Rec &o) const { return id == o.id && index == o.index && caller == o.caller; }
};
typedef std::map<Key, Rec> Model;

struct Rows {
    std::vector<uint32_t> key, id, index, caller;
    size_t n() const { return index.size(); }
    bool operator==(const Rows &o) const { return key == o.key && id == o.id && index == o.index && caller == o.caller; }
};

Key make_key(uint32_t tag, uint32_t i) {
    Key k;
    for (uint32_t q = 0; q < 8; q++) k[q] = (uint32_t)cvu_mix64(((uint64_t)tag << 40) ^ ((uint64_t)i << 8) ^ q);
    return k;
}

Rows make_rows(uint32_t tag, uint32_t n) {
    Rows r;
    for (uint32_t i = 0; i < n; i++) {
        const Key k = make_key(tag, i), id = make_key(tag + 1000, i);
        r.key.insert(r.key.end(), k.begin(), k.end());
        r.id.insert(r.id.end(), id.begin(), id.end());
        r.index.push_back(i % 5);
        r.caller.push_back(i * 2654435761u);
    }
    return r;
}

bool to_model(const Rows &r, Model *m) {
    m->clear();
    for (size_t i = 0; i < r.n(); i++) {
        Key k;
        Rec v;
        memcpy(k.data(), &r.key[8 * i], 32);
        memcpy(v.id.data(), &r.id[8 * i], 32);
        v.index = r.index[i];
        v.caller = r.caller[i];
        if (!m->insert({k, v}).second) return false;          // a key reported twice
    }
    return true;
}

int fail(const char *what, int order, uint64_t at) {
    fprintf(stderr, "uniq_snapshot_san: %s (order %d, at %llu)\n", what, order, (unsigned long long)at);
    return 1;
}

// one whole pass, max_entries records a call; false when a call fails or reports more than asked for
bool pass(void *s, uint64_t max_entries, int order, Rows *out, uint64_t *calls) {
    uint64_t cursor[2] = {0, 0}, n = 0;
    std::vector<uint32_t> key(8 * max_entries), id(8 * max_entries), index(max_entries), caller(max_entries);
    *out = Rows();
    *calls = 0;
    while (cursor[0] != kDone) {
        if (hus_snapshot(s, cursor, max_entries, order, key.data(), id.data(), index.data(), caller.data(), &n) != 0) return false;
        if (n > max_entries) return false;
        out->key.insert(out->key.end(), key.begin(), key.begin() + 8 * n);
        out->id.insert(out->id.end(), id.begin(), id.begin() + 8 * n);
        out->index.insert(out->index.end(), index.begin(), index.begin() + n);
        out->caller.insert(out->caller.end(), caller.begin(), caller.begin() + n);
        ++*calls;
    }
    n = 5;
    if (hus_snapshot(s, cursor, max_entries, order, key.data(), id.data(), index.data(), caller.data(), &n) != 0 || n != 0)
        return false;                                         // a finished cursor yields nothing
    return true;
}

int check_set(void *s, const Model &want, const uint64_t *chunks, size_t nchunks, int order) {
    Rows one, part;
    Model got;
    uint64_t calls = 0;
    if (!pass(s, want.empty() ? 1 : want.size(), order, &one, &calls)) return fail("whole pass", order, 0);
    if (!to_model(one, &got) || got != want) return fail("whole pass against the model", order, one.n());
    for (size_t c = 0; c < nchunks; c++) {
        if (!pass(s, chunks[c], order, &part, &calls)) return fail("chunked pass", order, chunks[c]);
        if (!(part == one)) return fail("chunks differ from the whole pass", order, chunks[c]);
    }
    return 0;
}

int load_rows(void *s, Rows &r, int order) {
    return hus_load(s, (uint32_t)r.n(), r.key.data(), r.id.data(), r.index.data(), r.caller.data(), order);
}

}  // namespace

int main() {
    unsigned cases = 0;
    for (int order = 0; order < 3; order++) {
        // wrap
        uint64_t wrapped = 0;
        const uint64_t small[4] = {1, 7, 8, 9};
        for (uint64_t seed = 0; seed < 64; seed++) {
            void *s = hus_open(8, seed, 1);
            Rows r = make_rows(1, 8);
            Model m;
            to_model(r, &m);
            if (load_rows(s, r, order) != 0) return fail("wrap: load", order, seed);
            uint64_t st[7];
            huq_stats(hus_set(s), st);
            if (st[2] != 16 || st[0] != 8) return fail("wrap: a full table of 16 slots", order, seed);
            wrapped += st[6];
            if (check_set(s, m, small, 4, order)) return 1;
            hus_close(s);
            cases++;
        }
        if (!wrapped) return fail("wrap: no probe passed the last slot", order, 0);
        // seams
        const uint64_t chunks[6] = {7, 64, 65, 256, 257, 1000}, one_by_one[1] = {1};
        void *a = hus_open(4096, 0xabcdef + (uint64_t)order, 77);
        Rows r = make_rows(2, 3000);
        Model m;
        to_model(r, &m);
        if (load_rows(a, r, order) != 0) return fail("seams: load", order, 0);
        if (check_set(a, m, chunks, 6, order)) return 1;
        void *c = hus_open(300, 3, 1);
        Rows r3 = make_rows(3, 300);
        Model m3;
        to_model(r3, &m3);
        if (load_rows(c, r3, order) != 0 || check_set(c, m3, one_by_one, 1, order)) return fail("one record a call", order, 0);
        hus_close(c);
        cases += 2;
        // install into another seed and a smaller capacity, over other contents
        Rows snap;
        uint64_t calls = 0;
        if (!pass(a, 3000, order, &snap, &calls)) return fail("install: snapshot", order, 0);
        void *b = hus_open(64, 0x1111, 5);
        Rows old = make_rows(4, 50);
        if (load_rows(b, old, order) != 0) return fail("install: old contents", order, 0);
        uint64_t cursor[2] = {0, 0}, n = 0;
        std::vector<uint32_t> k7(56), i7(56), x7(7), c7(7);
        if (hus_snapshot(b, cursor, 7, order, k7.data(), i7.data(), x7.data(), c7.data(), &n) != 0 || n != 7)
            return fail("install: first chunk", order, n);
        if (hus_install(b, snap.n(), snap.key.data(), snap.id.data(), snap.index.data(), snap.caller.data(), 0x2222, order) != 0)
            return fail("install", order, 0);
        if (hus_snapshot(b, cursor, 7, order, k7.data(), i7.data(), x7.data(), c7.data(), &n) != -3)
            return fail("install: the pass went on", order, 0);
        uint64_t st[7];
        huq_stats(hus_set(b), st);
        if (st[0] != 3000 || st[1] != 3000 || st[2] != 8192) return fail("install: resident, capacity, slots", order, st[1]);
        if (check_set(b, m, chunks, 6, order)) return 1;
        {   // every key, and the keys of the old contents
            std::vector<uint32_t> cid(8 * 3000), cix(3000), cc(3000);
            std::vector<uint8_t> found(3000);
            if (huq_lookup(hus_set(b), 3000, r.key.data(), order, found.data(), cid.data(), cix.data(), cc.data()) != 0)
                return fail("install: lookup", order, 0);
            for (uint32_t i = 0; i < 3000; i++)
                if (!found[i] || memcmp(&cid[8 * i], &r.id[8 * i], 32) != 0 || cix[i] != r.index[i] || cc[i] != r.caller[i])
                    return fail("install: record", order, i);
            if (huq_lookup(hus_set(b), 50, old.key.data(), order, found.data(), cid.data(), cix.data(), cc.data()) != 0)
                return fail("install: lookup of the old keys", order, 0);
            for (uint32_t i = 0; i < 50; i++)
                if (found[i]) return fail("install: an old key survived", order, i);
        }
        // a repeated key: the set as it was
        Rows bad = make_rows(5, 500);
        memcpy(&bad.key[8 * 499], &bad.key[8 * 17], 32);
        if (hus_install(b, bad.n(), bad.key.data(), bad.id.data(), bad.index.data(), bad.caller.data(), 0x3333, order) != -3)
            return fail("install: a repeated key accepted", order, 0);
        if (check_set(b, m, chunks, 1, order)) return 1;
        // clear, and the keys again
        cursor[0] = cursor[1] = 0;
        if (hus_snapshot(b, cursor, 7, order, k7.data(), i7.data(), x7.data(), c7.data(), &n) != 0) return fail("clear: chunk", order, 0);
        if (hus_clear(b) != 0) return fail("clear", order, 0);
        if (hus_snapshot(b, cursor, 7, order, k7.data(), i7.data(), x7.data(), c7.data(), &n) != -3)
            return fail("clear: the pass went on", order, 0);
        if (check_set(b, Model(), chunks, 2, order)) return 1;
        if (load_rows(b, r, order) != 0 || check_set(b, m, chunks, 1, order)) return fail("clear: the keys again", order, 0);
        hus_close(a);
        hus_close(b);
        cases += 3;
    }
    printf("ok %u\n", cases);
    return 0;
}
