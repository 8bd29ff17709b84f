// pmt_build_san.cpp — TEST INFRASTRUCTURE: a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer
// over the partial Merkle tree build core (cv_pmt_build.h through tests/pmt_build_harness.cpp).  It generates the
// exhaustive cases itself — every include subset of 0..8 leaves, through both include sources — and checks each
// built tree's round trip: the root against cv_merkle_root_inplace, the tree against cv_pmt_verify with the built
// root and the include list, the node count against the bound.  tests/test_pmt_build.py compiles it with
// -fsanitize=address,undefined and runs it; exit status 0 and "ok" on success.
#include <cstdio>

#include "pmt_build_harness.cpp"

static int fail(const char *what, uint32_t L, uint32_t mask, int src) {
    fprintf(stderr, "pmt_build_san: %s (L = %u, mask = 0x%x, source %d)\n", what, L, mask, src);
    return 1;
}

int main() {
    unsigned cases = 0;
    for (uint32_t L = 0; L <= 8; L++) {
        std::vector<uint8_t> leaf(32 * (size_t)L + 32);
        for (uint32_t i = 0; i < L; i++)
            for (int q = 0; q < 32; q++) leaf[32 * i + q] = (uint8_t)(17 * (i + 1) + 29 * q + (i << 5));
        const uint32_t txb[2] = {0, L};
        const size_t B = (size_t)cvb_bound(L);
        uint8_t want_root[32];
        const int has_root = cvb_root(L, leaf.data(), want_root);
        for (uint32_t mask = 0; mask < (1u << L); mask++) {
            std::vector<uint8_t> inc(32 * (size_t)L + 32), keep(L + 1, 0);
            uint32_t ninc = 0;
            for (uint32_t i = 0; i < L; i++)
                if (mask >> i & 1u) {
                    memcpy(&inc[32 * (size_t)ninc++], &leaf[32 * (size_t)i], 32);
                    keep[i] = 1;
                }
            const uint32_t ib[2] = {0, ninc};
            for (int src = 0; src < 2; src++) {
                // exactly the bound, so a write past the tree's own count lands outside the allocation
                std::vector<uint8_t> kind(B), hash(32 * B), ids(32), status(1);
                std::vector<uint32_t> left(B), right(B), tb(2);
                const uint32_t nn = cvb_build(1, leaf.data(), txb, src ? nullptr : inc.data(), src ? nullptr : ib,
                                              src ? keep.data() : nullptr, kind.data(), left.data(), right.data(),
                                              hash.data(), tb.data(), ids.data(), status.data());
                cases++;
                if (L == 0) {
                    if (status[0] != CV_PMTB_EMPTY || nn != 0 || has_root) return fail("empty transaction", L, mask, src);
                    continue;
                }
                if (status[0] != CV_PMTB_OK) return fail("status", L, mask, src);
                if (memcmp(ids.data(), want_root, 32) != 0) return fail("root", L, mask, src);
                if (nn == 0 || nn > B || tb[1] != nn) return fail("node count", L, mask, src);
                if (mask + 1 == (1u << L) && nn != B) return fail("all leaves included must reach the bound", L, mask, src);
                if (mask == 0 && nn != 1) return fail("no include must give one leaf", L, mask, src);
                if (cvb_verify(0, nn, kind.data(), left.data(), right.data(), hash.data(), ids.data(), inc.data(), 0, ninc) != 1)
                    return fail("round trip through cv_pmt_verify", L, mask, src);
            }
        }
    }
    printf("ok %u\n", cases);
    return 0;
}
