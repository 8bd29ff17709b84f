// uniq_san.cpp — TEST INFRASTRUCTURE: a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer over
// the uniqueness set's core (cv_uniq.h through tests/uniq_harness.cpp).  It generates its cases itself — random
// batches with carry-over on one small set that has to grow (0-5 states a request from a pool of 200 keys, repeats
// inside a request, empty and disabled requests), and a 300-request chain — and checks every output against a
// sequential std::map (InMemoryUniquenessProvider.commit, one request after another), in all three lane orders and
// with max_rounds 0, 1 and 8; after growth every record is looked up again.  Output arrays are sized exactly, so a
// write past them lands outside the allocation.  tests/test_uniq_cpu.py compiles it with
// -fsanitize=address,undefined and runs it; exit status 0 and "ok" on success.
#include <array>
#include <cstdio>
#include <map>

#include "uniq_harness.cpp"

namespace {

typedef std::array<uint32_t, 8> Key;
struct Rec {
    Key id;
    uint32_t index, caller;
};

uint64_t g_rng = 0x1234567887654321ull;
uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_rng >> 33) % n);
}

Key make_key(uint32_t tag, uint32_t i) {
    Key k;
    for (uint32_t q = 0; q < 8; q++) k[q] = (uint32_t)cvu_mix64(((uint64_t)tag << 40) ^ ((uint64_t)i << 8) ^ q);
    return k;
}

struct Batch {
    std::vector<uint32_t> key, begin, id, caller;
    std::vector<uint8_t> enable;
    uint32_t ntx = 0;
    void add(const std::vector<Key> &ks, const Key &txid, uint32_t who, bool on) {
        if (begin.empty()) begin.push_back(0);
        for (const Key &k : ks) key.insert(key.end(), k.begin(), k.end());
        begin.push_back((uint32_t)(key.size() / 8));
        id.insert(id.end(), txid.begin(), txid.end());
        caller.push_back(who);
        enable.push_back(on ? 1 : 0);
        ntx++;
    }
};

int fail(const char *what, int order, int rounds, uint32_t at) {
    fprintf(stderr, "uniq_san: %s (order %d, max_rounds %d, at %u)\n", what, order, rounds, at);
    return 1;
}

// commits b into the harness set and into the sequential model; 0 when every output agrees
int commit_and_check(void *h, std::map<Key, Rec> &model, const Batch &b, int order, int rounds) {
    const uint32_t S = b.begin[b.ntx];
    std::vector<uint8_t> st(b.ntx), sc(S);
    std::vector<uint32_t> cid(8 * (size_t)S), cix(S), cc(S);
    uint64_t stats[7];
    huq_stats(h, stats);
    if (stats[0] + S > stats[1] && huq_reserve(h, 2 * (stats[0] + S), order) != 0) return fail("reserve", order, rounds, 0);
    if (huq_commit(h, b.ntx, b.key.data(), b.begin.data(), b.id.data(), b.caller.data(), b.enable.data(), rounds, order,
                   st.data(), sc.data(), cid.data(), cix.data(), cc.data()) != 0)
        return fail("commit", order, rounds, 0);
    for (uint32_t t = 0; t < b.ntx; t++) {
        const uint32_t lo = b.begin[t], hi = b.begin[t + 1];
        if (!b.enable[t]) {
            if (st[t] != CVU_SKIPPED) return fail("skipped status", order, rounds, t);
            continue;
        }
        bool conflict = false;
        for (uint32_t i = lo; i < hi; i++) {
            Key k;
            memcpy(k.data(), &b.key[8 * (size_t)i], 32);
            const auto it = model.find(k);
            const bool hit = it != model.end();
            conflict |= hit;
            if (hit && (sc[i] != 1 || memcmp(&cid[8 * (size_t)i], it->second.id.data(), 32) != 0 ||
                        cix[i] != it->second.index || cc[i] != it->second.caller))
                return fail("conflict record", order, rounds, i);
        }
        if (st[t] != (conflict ? CVU_CONFLICT : CVU_OK)) return fail("status", order, rounds, t);
        for (uint32_t i = lo; i < hi; i++) {
            Key k;
            memcpy(k.data(), &b.key[8 * (size_t)i], 32);
            if (!conflict) {
                Rec r;
                memcpy(r.id.data(), &b.id[8 * (size_t)t], 32);
                r.index = i - lo;
                r.caller = b.caller[t];
                model[k] = r;
                if (sc[i] != 0) return fail("accepted state flagged", order, rounds, i);
            } else if (model.find(k) == model.end() && sc[i] != 0) {
                return fail("clean state flagged", order, rounds, i);
            }
        }
    }
    return 0;
}

int lookup_all(void *h, const std::map<Key, Rec> &model, int order) {
    const uint32_t n = (uint32_t)model.size();
    std::vector<uint32_t> key, cid(8 * (size_t)n), cix(n), cc(n);
    std::vector<uint8_t> found(n);
    for (const auto &kv : model) key.insert(key.end(), kv.first.begin(), kv.first.end());
    if (huq_lookup(h, n, key.data(), order, found.data(), cid.data(), cix.data(), cc.data()) != 0) return fail("lookup", order, 0, 0);
    uint32_t i = 0;
    for (const auto &kv : model) {
        if (!found[i] || memcmp(&cid[8 * (size_t)i], kv.second.id.data(), 32) != 0 || cix[i] != kv.second.index ||
            cc[i] != kv.second.caller)
            return fail("record after growth", order, 0, i);
        i++;
    }
    uint64_t stats[7];
    huq_stats(h, stats);
    return stats[0] == n ? 0 : fail("resident count", order, 0, n);
}

}  // namespace

int main() {
    unsigned batches = 0;
    const int round_caps[3] = {0, 1, 8};
    for (int order = 0; order < 3; order++)
        for (int rc = 0; rc < 3; rc++) {
            const int rounds = round_caps[rc];
            // random batches with carry-over, the set growing from 8 as it fills
            void *h = huq_open(8, 0x5eed0000u + (uint64_t)order);
            std::map<Key, Rec> model;
            for (uint32_t bi = 0; bi < 4; bi++) {
                Batch b;
                for (uint32_t t = 0; t < 300; t++) {
                    std::vector<Key> ks;
                    const uint32_t n = rnd(6);
                    for (uint32_t j = 0; j < n; j++) ks.push_back(make_key(1, rnd(200)));
                    if (n && rnd(5) == 0) ks.push_back(ks[rnd(n)]);
                    b.add(ks, make_key(2, 300 * bi + t), rnd(5), rnd(10) != 0);
                }
                if (commit_and_check(h, model, b, order, rounds)) return 1;
                if (lookup_all(h, model, order)) return 1;
                batches++;
            }
            huq_close(h);
            // the chain: request t holds keys t and t + 1
            h = huq_open(600, 77);
            model.clear();
            Batch c;
            for (uint32_t t = 0; t < 300; t++) c.add({make_key(3, t), make_key(3, t + 1)}, make_key(4, t), t % 3, true);
            if (commit_and_check(h, model, c, order, rounds)) return 1;
            if (model.size() != 300) return fail("chain: 150 requests of 2 states", order, rounds, (uint32_t)model.size());
            if (huq_reserve(h, 5000, order) != 0 || lookup_all(h, model, order)) return 1;
            huq_close(h);
            batches++;
        }
    printf("ok %u\n", batches);
    return 0;
}
