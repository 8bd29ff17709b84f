// tearoff_san.cpp — TEST INFRASTRUCTURE: a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer over
// the per-lane decisions of cv_filtered_verify and cv_tearoff_sign_batch (cv_tearoff.h through
// tests/tearoff_harness.cpp).  It generates its cases itself — random batches of 0-4 filtered leaves a tear-off over
// one-node trees (an IncludedLeaf that carries the first leaf's hash, a wrong hash, or an unknown kind), leaf_pre
// switched on at random in every class — runs the chain leaf digests -> check bytes -> tree verify -> gate ->
// compaction and checks every output against a plain sequential model, in all three lane orders, with and without
// leaf_pre.  Every array is sized exactly (the arena to whole dwords: the SHA-256 code reads aligned dwords), so a read
// or write past it lands outside the allocation.  tests/test_tearoff_cpu.py compiles it with
// -fsanitize=address,undefined and runs it; exit status 0 and "ok" on success.
#include <cstdio>

#include "tearoff_harness.cpp"

namespace {

uint64_t g_rng = 0x0123456789abcdefull;
uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_rng >> 33) % n);
}

int fail(const char *what, int order, uint32_t at) {
    fprintf(stderr, "tearoff_san: %s (order %d, at %u)\n", what, order, at);
    return 1;
}

int one_batch(uint32_t ntx, int order, bool with_pre) {
    std::vector<uint32_t> txb(ntx + 1, 0), tb(ntx + 1, 0), len;
    std::vector<uint64_t> off;
    std::vector<uint8_t> arena;
    for (uint32_t t = 0; t < ntx; t++) {
        const uint32_t k = rnd(8) == 0 ? 0 : 1 + rnd(8) / 5 * (1 + rnd(3));      // mostly one leaf
        for (uint32_t j = 0; j < k; j++) {
            const uint32_t n = rnd(4) == 0 ? 55 + rnd(12) : rnd(140);             // around the padding seam, and any
            off.push_back(arena.size());
            len.push_back(n);
            for (uint32_t q = 0; q < n; q++) arena.push_back((uint8_t)rnd(256));
        }
        txb[t + 1] = txb[t] + k;
        tb[t + 1] = tb[t] + 1;
    }
    while (arena.size() % 4) arena.push_back(0);
    const uint32_t nl = txb[ntx];
    std::vector<uint32_t> dig(8 * (size_t)nl), chk(8 * (size_t)nl);
    htf_leaf_digests(nl, arena.data(), off.data(), len.data(), dig.data());
    htf_check(nl, dig.data(), order, chk.data());
    const uint8_t *cb = reinterpret_cast<const uint8_t *>(chk.data());
    for (uint32_t i = 0; i < nl; i++)
        for (int q = 0; q < 8; q++) {
            const uint32_t w = dig[8 * (size_t)i + q];
            const uint8_t *b = cb + 32 * (size_t)i + 4 * q;
            if (b[0] != (w >> 24) || b[1] != ((w >> 16) & 255) || b[2] != ((w >> 8) & 255) || b[3] != (w & 255))
                return fail("check", order, i);
        }
    // one node a tree; want_v / want_st: what PartialMerkleTree.verify gives over the filtered hashes
    std::vector<uint8_t> kind(ntx), hash(32 * (size_t)ntx), root(32 * (size_t)ntx), want_v(ntx), want_st(ntx);
    std::vector<uint32_t> zero(ntx, 0);
    for (uint32_t t = 0; t < ntx; t++) {
        const uint32_t k = txb[t + 1] - txb[t], how = rnd(8);
        kind[t] = how == 0 ? 9 : CV_PMT_INCLUDED;
        for (int q = 0; q < 32; q++) hash[32 * (size_t)t + q] = k ? cb[32 * (size_t)txb[t] + q] : (uint8_t)rnd(256);
        if (how == 1) hash[32 * (size_t)t + rnd(32)] ^= 1u << rnd(8);
        memcpy(&root[32 * (size_t)t], &hash[32 * (size_t)t], 32);
        if (how == 2) root[32 * (size_t)t + rnd(32)] ^= 1u << rnd(8);
        want_st[t] = how == 0 ? 2 : 0;
        want_v[t] = how > 2 && k == 1;
    }
    std::vector<uint8_t> v(ntx), st(ntx);
    htf_verify(ntx, ntx, kind.data(), zero.data(), zero.data(), hash.data(), tb.data(), root.data(), cb, txb.data(),
               v.data(), st.data());
    for (uint32_t t = 0; t < ntx; t++)
        if (v[t] != want_v[t] || st[t] != want_st[t]) return fail("verify", order, t);
    std::vector<uint8_t> pre(nl);
    for (uint8_t &p : pre) p = rnd(6) == 0 ? (uint8_t)(1 + rnd(3)) : 0;
    std::vector<uint8_t> fv(ntx), fst(ntx), out(ntx);
    std::vector<uint32_t> fb(ntx);
    htf_gate(ntx, txb.data(), v.data(), st.data(), with_pre ? pre.data() : nullptr, order, fv.data(), fst.data(), out.data(),
             fb.data());
    uint32_t want_count = 0;
    for (uint32_t t = 0; t < ntx; t++) {
        uint32_t o = CVT_SUCCESS, bad = CVT_NO_LEAF, wv = 0, ws = 0;
        if (txb[t] == txb[t + 1]) o = CVT_NO_LEAVES, ws = CVT_PMT_NO_INCLUDED;
        else if (want_st[t]) o = CVT_MALFORMED, ws = CVT_PMT_MALFORMED;
        else if (!want_v[t]) o = CVT_VERIFY_FAILED;
        else {
            wv = 1;
            for (uint32_t cls = 1; cls <= 3 && with_pre && o == CVT_SUCCESS; cls++)
                for (uint32_t i = txb[t]; i < txb[t + 1] && o == CVT_SUCCESS; i++)
                    if (pre[i] == cls) o = CVT_VERIFY_FAILED + cls, bad = i;
        }
        if (out[t] != o || fb[t] != bad || fv[t] != wv || fst[t] != ws) return fail("gate", order, t);
        want_count += o == CVT_SUCCESS;
    }
    // the list arrays hold exactly the accepted tear-offs: a place past the count is a write past the allocation
    std::vector<uint32_t> list(want_count), slen(want_count);
    std::vector<uint64_t> soff(want_count);
    const uint32_t count = htf_compact(ntx, out.data(), order, list.data(), soff.data(), slen.data());
    if (count != want_count) return fail("count", order, count);
    uint32_t j = 0;
    for (uint32_t t = 0; t < ntx; t++)
        if (out[t] == CVT_SUCCESS) {
            if (list[j] != t || soff[j] != 32ull * t || slen[j] != 32) return fail("list", order, t);
            j++;
        }
    return 0;
}

}  // namespace

int main() {
    unsigned batches = 0;
    const uint32_t sizes[] = {1, 2, 63, 64, 65, 130, 257, 1500};
    for (int order = 0; order < 3; order++)
        for (uint32_t ntx : sizes)
            for (int with_pre = 0; with_pre < 2; with_pre++) {
                if (one_batch(ntx, order, with_pre != 0)) return 1;
                batches++;
            }
    printf("ok %u\n", batches);
    return 0;
}
