// keystore_harness.cpp — TEST INFRASTRUCTURE: the device key store's per-lane core (corda_amd/csrc/cv_keystore.h;
// __host__ __device__) on the CPU, for tests/test_keystore_cpu.py, which builds this file into
// tests/_build/libcvkeystore.so, and for tests/keystore_san.cpp, which includes it.
//
// A HStore is what cv_keystore is in cv_api_keystore.cpp, in host memory; hks_add / hks_lookup / hks_reserve /
// hks_tx_gate run the steps the launchers of cv_kernels.hip enqueue (cvk_ks_add, _lookup, _rehash, _tx_gate), each
// step's lanes ONE AFTER ANOTHER in the order `order` names: 0 ascending, 1 descending, 2 one fixed shuffle.  The
// results must not depend on it.  Seeds are expanded with cv_key_expand (cv_verify.h) as the expansion kernel's lanes
// do.  hks_record hands out a slot's record: the harness is no entry point of the library, which never does.
// Return codes as the C-ABI's: 0, -2 (a probe ran out), -4.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../corda_amd/csrc/cv_verify.h"
#include "../corda_amd/csrc/cv_keystore.h"

namespace {

struct HStore {
    std::vector<uint32_t> mem;
    CvKeyTable T{};
    size_t capacity = 0, resident = 0;
    uint64_t probe = 0;
};

// a zeroed table for `capacity` keys in mem: the library's size (cv_table.h) and carve-up (cv_keystore.h)
void carve(std::vector<uint32_t> &mem, size_t capacity, uint64_t seed, CvKeyTable *T) {
    const size_t slots = (size_t)cv_table_slots(capacity, 16);
    mem.assign(CKS_SLOT_BYTES * slots / 4, 0);
    *T = cks_carve(mem.data(), slots, seed);
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

int fold(HStore *h, const uint32_t *dstat) {
    h->probe = dstat[CKS_D_MAXPROBE];
    return dstat[CKS_D_ERROR] ? -2 : 0;
}

}  // namespace

extern "C" {

void *hks_open(uint64_t capacity, uint64_t seed) {
    HStore *h = new HStore();
    h->capacity = capacity ? capacity : 1;
    carve(h->mem, h->capacity, seed, &h->T);
    return h;
}

void hks_close(void *p) { delete static_cast<HStore *>(p); }

void hks_stats(void *p, uint64_t out[4]) {
    HStore *h = static_cast<HStore *>(p);
    const uint64_t v[4] = {h->resident, h->capacity, (uint64_t)h->T.mask + 1, h->probe};
    memcpy(out, v, sizeof v);
}

int hks_reserve(void *p, uint64_t capacity, int order) {
    HStore *h = static_cast<HStore *>(p);
    if (capacity <= h->capacity) return 0;
    if (cv_table_slots(capacity, 16) == (uint64_t)h->T.mask + 1) {
        h->capacity = capacity;
        return 0;
    }
    std::vector<uint32_t> mem;
    CvKeyTable to{};
    carve(mem, capacity, h->T.seed, &to);
    uint32_t dstat[CKS_D_WORDS] = {};
    for (uint32_t s : lanes((size_t)h->T.mask + 1, order)) cks_rehash(h->T, to, s, dstat);
    const int rc = fold(h, dstat);
    if (rc) return rc;
    h->mem.swap(mem);
    h->T = to;
    h->capacity = capacity;
    return 0;
}

// cv_keystore_add: seed (n * 8 words) -> pk_out (n * 8 words), status[n]
int hks_add(void *p, uint32_t n, const uint32_t *seed, int order, uint32_t *pk_out, uint8_t *status) {
    HStore *h = static_cast<HStore *>(p);
    if (n == 0) return 0;
    if (h->resident + n > h->capacity) return -4;
    const std::vector<uint32_t> ln = lanes(n, order);
    std::vector<uint32_t> rec((size_t)CKS_REC_WORDS * n);
    for (uint32_t i : ln) {                                       // cv_ks_expand_kernel
        uint32_t *r = rec.data() + (size_t)CKS_REC_WORDS * i;
        cv_key_expand(seed + 8 * (size_t)i, r + CKS_REC_A, r + CKS_REC_PREFIX, r + CKS_REC_ABYTE, CV_BTAB_H);
        memcpy(pk_out + 8 * (size_t)i, r + CKS_REC_ABYTE, 32);
    }
    const CvdLayout L = cvd_layout(n);
    std::vector<uint32_t> ws((size_t)(L.bytes / 4), 0);
    const CvDedupe D = cvd_args(n, pk_out, nullptr, nullptr, nullptr, ws.data(), 0x5eedull ^ h->T.seed, L);
    memset(D.tab, 0xff, 4 * (size_t)L.slots + 4 * CVD_STAT_WORDS);
    uint32_t dstat[CKS_D_WORDS] = {};
    for (uint32_t i : ln) cvd_insert(D, i);                       // cv_dedupe_insert_kernel
    for (uint32_t i : ln) cks_classify(h->T, D, i, status, dstat);
    for (uint32_t i : ln) cks_put(h->T, D, i, rec.data(), status, dstat);
    h->resident += dstat[CKS_D_ADDED];
    return fold(h, dstat);
}

// cv_keystore_contains (present = 1) and the lookup ahead of signing (present = 0): slot and flag may be null
int hks_lookup(void *p, uint32_t n, const uint32_t *pk, int order, uint32_t *slot, uint8_t *flag, int present) {
    HStore *h = static_cast<HStore *>(p);
    uint32_t dstat[CKS_D_WORDS] = {};
    for (uint32_t i : lanes(n, order)) cks_lookup(h->T, pk, i, slot, flag, (uint8_t)present, dstat);
    return fold(h, dstat);
}

// the 24 words of a slot's record (zero for CKS_NONE or a slot past the table)
void hks_record(void *p, uint32_t slot, uint32_t *out) {
    HStore *h = static_cast<HStore *>(p);
    memset(out, 0, 4 * CKS_REC_WORDS);
    if (slot <= h->T.mask && h->T.occ[slot]) memcpy(out, h->T.rec + (size_t)CKS_REC_WORDS * slot, 4 * CKS_REC_WORDS);
}

// the gate of cv_sign_transactions: slot / off / len per key, tx_status and first_bad per transaction
int hks_tx_gate(void *p, uint32_t ntx, const uint32_t *leaf_begin, const uint32_t *sig_begin, const uint32_t *pk, int order,
                uint32_t *slot, uint64_t *off, uint32_t *len, uint8_t *tx_status, uint32_t *first_bad) {
    HStore *h = static_cast<HStore *>(p);
    uint32_t dstat[CKS_D_WORDS] = {};
    CvKeyTx X{};
    X.ntx = ntx;
    X.leaf_begin = leaf_begin;
    X.sig_begin = sig_begin;
    X.pk = pk;
    X.slot = slot;
    X.off = off;
    X.len = len;
    X.tx_status = tx_status;
    X.first_bad = first_bad;
    X.dstat = dstat;
    for (uint32_t t : lanes(ntx, order)) cks_tx_gate(h->T, X, t);
    return fold(h, dstat);
}

}  // extern "C"
