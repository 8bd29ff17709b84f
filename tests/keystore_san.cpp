// keystore_san.cpp — TEST INFRASTRUCTURE: a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer over
// the key store's core (cv_keystore.h through tests/keystore_harness.cpp).  It generates its cases itself — calls of
// 1-40 seeds drawn with repeats from a pool of 90 on one small store that has to grow, then lookups of the whole pool
// and 200 transactions of 0-4 keys through the gate — and checks every output against a sequential std::map (one
// freshKey / toPrivate / signWith after another), in all three lane orders.  Output arrays are sized exactly, so a
// write past them lands outside the allocation.  tests/test_keystore_cpu.py compiles it with
// -fsanitize=address,undefined and runs it; exit status 0 and "ok" on success.
#include <algorithm>
#include <array>
#include <cstdio>
#include <map>

#include "keystore_harness.cpp"

namespace {

typedef std::array<uint32_t, 8> Key;

uint64_t g_rng = 0x1234567887654321ull;
uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_rng >> 33) % n);
}

Key make_seed(uint32_t i) {
    Key k;
    for (uint32_t q = 0; q < 8; q++) k[q] = (uint32_t)cvu_mix64(((uint64_t)i << 8) ^ q ^ 0xabcdef0000ull);
    return k;
}

int fail(const char *what, int order, uint32_t at) {
    fprintf(stderr, "keystore_san: %s (order %d, at %u)\n", what, order, at);
    return 1;
}

const uint32_t kPool = 90;

}  // namespace

int main() {
    unsigned calls = 0;
    for (int order = 0; order < 3; order++) {
        void *h = hks_open(8, 0x5eed0000u + (uint64_t)order);
        std::map<Key, Key> model;                                   // public key -> seed
        std::vector<Key> pool_pk(kPool);
        std::vector<uint8_t> known(kPool, 0);
        for (uint32_t c = 0; c < 12; c++) {
            const uint32_t n = 1 + rnd(40);
            std::vector<uint32_t> pick(n), seed(8 * (size_t)n), pk(8 * (size_t)n);
            std::vector<uint8_t> st(n);
            for (uint32_t i = 0; i < n; i++) {
                pick[i] = rnd(c < 6 ? 45 : kPool);
                const Key s = make_seed(pick[i]);
                memcpy(&seed[8 * (size_t)i], s.data(), 32);
            }
            uint64_t stats[4];
            hks_stats(h, stats);
            if (stats[0] + n > stats[1]) {                          // refused whole, outputs untouched; then grown
                st.assign(n, 0xee);
                if (hks_add(h, n, seed.data(), order, pk.data(), st.data()) != -4) return fail("capacity not enforced", order, c);
                for (uint32_t i = 0; i < n; i++)
                    if (st[i] != 0xee || pk[8 * (size_t)i] != 0) return fail("refused call wrote an output", order, i);
                if (hks_reserve(h, 2 * (stats[0] + n), order) != 0) return fail("reserve", order, c);
            }
            if (hks_add(h, n, seed.data(), order, pk.data(), st.data()) != 0) return fail("add", order, c);
            for (uint32_t i = 0; i < n; i++) {
                Key k, s = make_seed(pick[i]);
                memcpy(k.data(), &pk[8 * (size_t)i], 32);
                if (known[pick[i]] && pool_pk[pick[i]] != k) return fail("pk_out changed for a seed", order, i);
                pool_pk[pick[i]] = k;
                known[pick[i]] = 1;
                const bool fresh = model.find(k) == model.end();
                if (st[i] != (fresh ? CKS_ADDED : CKS_PRESENT)) return fail("add status", order, i);
                if (fresh) model[k] = s;
            }
            hks_stats(h, stats);
            if (stats[0] != model.size()) return fail("resident count", order, c);
            calls++;
        }
        // every key of the pool: found iff the model holds it, and the slot's record carries the key
        std::vector<uint32_t> pk(8 * (size_t)kPool), slot(kPool);
        std::vector<uint8_t> found(kPool);
        for (uint32_t i = 0; i < kPool; i++) {
            if (!known[i]) {                                        // never added: its public key is unknown, ask for the seed's bytes
                const Key s = make_seed(i);
                pool_pk[i] = s;
            }
            memcpy(&pk[8 * (size_t)i], pool_pk[i].data(), 32);
        }
        if (hks_lookup(h, kPool, pk.data(), order, slot.data(), found.data(), 1) != 0) return fail("lookup", order, 0);
        for (uint32_t i = 0; i < kPool; i++) {
            const bool want = model.find(pool_pk[i]) != model.end();
            if ((found[i] != 0) != want || (slot[i] != CKS_NONE) != want) return fail("found", order, i);
            uint32_t rec[CKS_REC_WORDS];
            hks_record(h, slot[i], rec);
            if (want && memcmp(rec + CKS_REC_ABYTE, pool_pk[i].data(), 32) != 0) return fail("record", order, i);
        }
        // the gate: transactions over the pool's keys (absent ones included), repeats, empty transactions
        const uint32_t ntx = 200;
        std::vector<uint32_t> lb(1, 0), sb(1, 0), tpk;
        for (uint32_t t = 0; t < ntx; t++) {
            const uint32_t nk = rnd(5);
            for (uint32_t j = 0; j < nk; j++) {
                const Key &k = pool_pk[rnd(kPool)];
                tpk.insert(tpk.end(), k.begin(), k.end());
            }
            if (nk >= 2 && rnd(4) == 0) memcpy(&tpk[tpk.size() - 8], &tpk[tpk.size() - 8 * nk], 32);
            lb.push_back(lb.back() + (rnd(5) == 0 ? 0 : 1 + rnd(4)));
            sb.push_back(sb.back() + nk);
        }
        const uint32_t ns = sb.back();
        std::vector<uint32_t> gslot(ns), glen(ns), fb(ntx);
        std::vector<uint64_t> goff(ns);
        std::vector<uint8_t> gst(ntx);
        if (hks_tx_gate(h, ntx, lb.data(), sb.data(), tpk.data(), order, gslot.data(), goff.data(), glen.data(), gst.data(),
                        fb.data()) != 0)
            return fail("gate", order, 0);
        for (uint32_t t = 0; t < ntx; t++) {
            const bool empty = lb[t + 1] == lb[t];
            uint32_t st = CKS_ST_OK, bad = CKS_NONE;
            std::vector<Key> signed_by;
            for (uint32_t j = sb[t]; j < sb[t + 1] && st == CKS_ST_OK; j++) {
                Key k;
                memcpy(k.data(), &tpk[8 * (size_t)j], 32);
                if (model.find(k) == model.end()) st = CKS_ST_NO_KEY;
                else if (std::find(signed_by.begin(), signed_by.end(), k) != signed_by.end()) st = CKS_ST_ALREADY_SIGNED;
                else if (empty) st = CKS_ST_EMPTY;
                if (st != CKS_ST_OK) bad = j - sb[t];
                signed_by.push_back(k);
            }
            if (st == CKS_ST_OK && empty) st = CKS_ST_EMPTY, bad = 0;
            if (gst[t] != st || fb[t] != bad) return fail("gate status", order, t);
            for (uint32_t j = sb[t]; j < sb[t + 1]; j++) {
                if (goff[j] != 32ull * t || glen[j] != 32) return fail("gate message", order, j);
                if ((gslot[j] == CKS_NONE) != (st != CKS_ST_OK)) return fail("gate slot", order, j);
                uint32_t rec[CKS_REC_WORDS];
                hks_record(h, gslot[j], rec);
                if (st == CKS_ST_OK && memcmp(rec + CKS_REC_ABYTE, &tpk[8 * (size_t)j], 32) != 0) return fail("gate record", order, j);
            }
        }
        hks_close(h);
        calls++;
    }
    printf("ok %u\n", calls);
    return 0;
}
