// notary_san.cpp — TEST INFRASTRUCTURE: a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer over
// the per-lane decisions of cv_notarise_batch (cv_notary.h through tests/notary_harness.cpp).  It generates its cases
// itself — random batches of 0-5 signatures a transaction (so ranges straddle the bitmap's words) with every gating
// condition switched on at random, random uniqueness statuses, random state -> leaf lists — and checks every output
// against a plain sequential model, in all three lane orders, validating and not.  Every array is sized exactly, so a
// read or write past it lands outside the allocation.  tests/test_notary_cpu.py compiles it with
// -fsanitize=address,undefined and runs it; exit status 0 and "ok" on success.
#include <cstdio>

#include "notary_harness.cpp"

namespace {

uint64_t g_rng = 0x0123456789abcdefull;
uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_rng >> 33) % n);
}

int fail(const char *what, int order, int validating, uint32_t at) {
    fprintf(stderr, "notary_san: %s (order %d, validating %d, at %u)\n", what, order, validating, at);
    return 1;
}

int one_batch(uint32_t ntx, int validating, int order, bool with_pre) {
    std::vector<uint8_t> mst(ntx), tpre(ntx), ck(ntx), ust(ntx);
    std::vector<uint32_t> id(8 * (size_t)ntx), claimed(8 * (size_t)ntx), tsb(ntx + 1, 0);
    for (uint32_t t = 0; t < ntx; t++) {
        mst[t] = rnd(8) == 0;
        tpre[t] = rnd(8) == 0 ? (uint8_t)(1 + rnd(200)) : 0;
        ck[t] = rnd(3) == 0 ? (uint8_t)rnd(4) : 0;
        ust[t] = (uint8_t)rnd(3);
        for (int q = 0; q < 8; q++) id[8 * (size_t)t + q] = claimed[8 * (size_t)t + q] = rnd(0xffffffffu);
        if (rnd(8) == 0) claimed[8 * (size_t)t + rnd(8)] ^= 1u << rnd(32);
        tsb[t + 1] = tsb[t] + (validating ? rnd(6) : 0);
    }
    const uint32_t nsig = tsb[ntx];
    std::vector<uint64_t> bm((nsig + 63) / 64, 0);
    std::vector<uint8_t> sst(nsig), spre(nsig);
    for (uint32_t i = 0; i < nsig; i++) {
        if (rnd(6) != 0) bm[i >> 6] |= 1ull << (i & 63);
        sst[i] = rnd(4) == 0;
        spre[i] = rnd(10) == 0 ? (uint8_t)(1 + rnd(2)) : 0;
    }
    std::vector<uint8_t> pre(ntx), en(ntx), out(ntx);
    std::vector<uint32_t> fb(ntx);
    hnt_gate(ntx, validating, mst.data(), id.data(), claimed.data(), with_pre ? tpre.data() : nullptr, tsb.data(), bm.data(),
             sst.data(), with_pre ? spre.data() : nullptr, ck.data(), order, pre.data(), en.data(), fb.data());
    uint32_t want_count = 0;
    std::vector<uint8_t> want(ntx);
    for (uint32_t t = 0; t < ntx; t++) {
        uint32_t o = CVN_SUCCESS, bad = CVN_NO_SIG;
        if (mst[t]) o = CVN_EMPTY;
        else if (memcmp(&id[8 * (size_t)t], &claimed[8 * (size_t)t], 32) != 0) o = CVN_ID_MISMATCH;
        else if (with_pre && tpre[t]) o = CVN_TIMESTAMP_INVALID;
        else if (validating) {
            for (uint32_t i = tsb[t]; i < tsb[t + 1] && bad == CVN_NO_SIG; i++) {
                const uint8_t p = with_pre ? spre[i] : 0;
                if (p || !((bm[i >> 6] >> (i & 63)) & 1)) {
                    bad = i;
                    o = p == 2 || (p == 0 && sst[i] == 1) ? CVN_BAD_KEY : CVN_TX_INVALID;
                }
            }
            if (bad == CVN_NO_SIG) {
                if (tsb[t] == tsb[t + 1]) o = CVN_TX_INVALID;
                else if (ck[t] == 3) o = CVN_MALFORMED;
                else if (ck[t] == 2) o = CVN_SIGNATURES_MISSING;
            }
        }
        if (pre[t] != o || en[t] != (o == CVN_SUCCESS) || fb[t] != bad) return fail("gate", order, validating, t);
        want[t] = (uint8_t)(o == CVN_SUCCESS && ust[t] == 1 ? CVN_CONFLICT : o);
        want_count += want[t] == CVN_SUCCESS;
    }
    // the list arrays hold exactly the accepted transactions: a place past the count is a write past the allocation
    std::vector<uint32_t> list(want_count), slen(want_count);
    std::vector<uint64_t> soff(want_count);
    const uint32_t count = hnt_final(ntx, pre.data(), ust.data(), order, out.data(), list.data(), soff.data(), slen.data());
    if (count != want_count) return fail("count", order, validating, count);
    uint32_t j = 0;
    for (uint32_t t = 0; t < ntx; t++) {
        if (out[t] != want[t]) return fail("outcome", order, validating, t);
        if (want[t] == CVN_SUCCESS) {
            if (list[j] != t || soff[j] != 32ull * t || slen[j] != 32) return fail("list", order, validating, t);
            j++;
        }
    }
    // gather: random leaf lists over random digests
    const uint32_t nleaves = 1 + rnd(300), nstates = rnd(400);
    std::vector<uint32_t> dig(8 * (size_t)nleaves), sl(nstates), key(8 * (size_t)nstates);
    for (uint32_t &w : dig) w = rnd(0xffffffffu);
    for (uint32_t &l : sl) l = rnd(nleaves);
    hnt_gather(nstates, dig.data(), sl.data(), order, key.data());
    for (uint32_t i = 0; i < nstates; i++)
        for (int q = 0; q < 8; q++) {
            const uint8_t *b = reinterpret_cast<const uint8_t *>(&key[8 * (size_t)i + q]);
            const uint32_t w = dig[8 * (size_t)sl[i] + q];
            if (b[0] != (w >> 24) || b[1] != ((w >> 16) & 255) || b[2] != ((w >> 8) & 255) || b[3] != (w & 255))
                return fail("gather", order, validating, i);
        }
    return 0;
}

}  // namespace

int main() {
    unsigned batches = 0;
    const uint32_t sizes[] = {1, 2, 63, 64, 65, 130, 257, 1500};
    for (int order = 0; order < 3; order++)
        for (int validating = 0; validating < 2; validating++)
            for (uint32_t ntx : sizes)
                for (int with_pre = 0; with_pre < 2; with_pre++) {
                    if (one_batch(ntx, validating, order, with_pre != 0)) return 1;
                    batches++;
                }
    printf("ok %u\n", batches);
    return 0;
}
