// resolve_san.cpp — TEST INFRASTRUCTURE: a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer over
// the graph half of cv_resolve_batch (cv_resolve.h through tests/resolve_harness.cpp): the three lane steps and the
// library's host order and walk.  It generates its cases itself — random graphs with inputs inside and outside the
// batch, self-references and cycles, indices at and past the output counts, repeated ids, mismatched ids, every
// signature condition switched on at random, tables at the library's size and at the smallest size that leaves a slot
// empty (nearly full: probes chain and wrap) — and checks every output against a plain sequential model (std::map keyed by the id bytes, visit()
// recursive as the reference's), in all lane orders.  Every array is sized exactly, so a read or write past it lands
// outside the allocation.  tests/test_resolve_cpu.py compiles it with -fsanitize=address,undefined and runs it; exit
// status 0 and "ok" on success.
#include <array>
#include <cstdio>
#include <map>
#include <set>

#include "resolve_harness.cpp"

namespace {

typedef std::array<uint32_t, 8> Id;

uint64_t g_rng = 0x0123456789abcdefull;
uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_rng >> 33) % n);
}

int fail(const char *what, int order, uint32_t ntx, uint32_t at) {
    fprintf(stderr, "resolve_san: %s (order %d, ntx %u, at %u)\n", what, order, ntx, at);
    return 1;
}

struct Model {
    uint32_t ntx;
    const std::vector<Id> &id;
    const std::vector<uint32_t> &tib;
    const std::vector<Id> &hash;
    std::map<Id, std::vector<uint32_t>> forward;
    std::set<Id> visited;
    std::vector<uint32_t> result;
    void visit(uint32_t t) {
        if (visited.count(id[t])) return;
        visited.insert(id[t]);
        auto it = forward.find(id[t]);
        if (it != forward.end())
            for (uint32_t d : it->second) visit(d);
        result.push_back(t);
    }
    void sort() {
        for (uint32_t t = 0; t < ntx; t++)
            for (uint32_t i = tib[t]; i < tib[t + 1]; i++) {
                std::vector<uint32_t> &v = forward[hash[i]];
                if (v.empty() || v.back() != t) v.push_back(t);
            }
        for (uint32_t t = 0; t < ntx; t++) visit(t);
        std::reverse(result.begin(), result.end());
    }
};

int one_batch(uint32_t ntx, int order, bool tiny, bool clean) {
    std::vector<Id> id(ntx), claimed(ntx);
    std::vector<uint8_t> mst(ntx), ck(ntx);
    std::vector<uint32_t> tsb(ntx + 1, 0), tib(ntx + 1, 0), nout(ntx);
    for (uint32_t t = 0; t < ntx; t++) {
        for (uint32_t &w : id[t]) w = rnd(0xffffffffu);
        if (!clean && t && rnd(40) == 0) id[t] = id[rnd(t)];                 // a repeated id
        claimed[t] = id[t];
        if (!clean && rnd(50) == 0) claimed[t][rnd(8)] ^= 1u << rnd(32);     // a mismatch
        mst[t] = !clean && rnd(60) == 0;
        ck[t] = rnd(6) == 0 ? (uint8_t)rnd(4) : 0;
        nout[t] = rnd(4);
        tsb[t + 1] = tsb[t] + rnd(4);
        tib[t + 1] = tib[t] + rnd(5);
    }
    const uint32_t nsig = tsb[ntx], nin = tib[ntx];
    std::vector<uint64_t> bm((nsig + 63) / 64, 0);
    std::vector<uint8_t> sst(nsig), spre(nsig);
    for (uint32_t i = 0; i < nsig; i++) {
        if (rnd(12) != 0) bm[i >> 6] |= 1ull << (i & 63);
        sst[i] = rnd(4) == 0;
        spre[i] = rnd(20) == 0 ? (uint8_t)(1 + rnd(2)) : 0;
    }
    std::vector<Id> hash(nin);
    std::vector<uint32_t> index(nin);
    for (uint32_t i = 0; i < nin; i++) {
        if (rnd(4) == 0)
            for (uint32_t &w : hash[i]) w = rnd(0xffffffffu);                // outside the batch
        else
            hash[i] = claimed[rnd(ntx)];                                     // any transaction: itself, cycles
        index[i] = rnd(8) == 0 ? 0xffffffffu : rnd(4);
    }
    std::vector<uint8_t> outcome(ntx), ist(nin);
    std::vector<uint32_t> fb(ntx), bin(ntx), dep(nin), ord(ntx), graph(CVR_G_WORDS);
    const int rc = hrs_run(ntx, nin, claimed[0].data(), tib.data(), nin ? hash[0].data() : nullptr, index.data(),
                           nout.data(), mst.data(), id[0].data(), tsb.data(), bm.data(), sst.data(), spre.data(), ck.data(),
                           0x1234567 + ntx, tiny ? hrs_slots((ntx + 2) / 2) : 0, order, outcome.data(), fb.data(),
                           bin.data(), dep.data(), ist.data(), ord.data(), graph.data());
    if (rc != 0) return fail("hrs_run", order, ntx, (uint32_t)-rc);

    // the sequential model
    std::map<Id, uint32_t> first;
    std::map<Id, uint32_t> count;
    for (uint32_t t = 0; t < ntx; t++) {
        first.insert({claimed[t], t});
        count[claimed[t]]++;
    }
    uint32_t ext = 0, badid = CVR_NONE, dup = CVR_NONE;
    std::vector<uint32_t> pre(ntx);
    for (uint32_t t = 0; t < ntx; t++) {
        uint32_t o = CVR_OK, bad = CVN_NO_SIG, b_in = CVR_NONE;
        for (uint32_t i = tib[t]; i < tib[t + 1]; i++) {
            auto it = first.find(hash[i]);
            const uint32_t d = it == first.end() ? CVR_NONE : it->second;
            const uint8_t st = d == CVR_NONE ? 0 : index[i] < nout[d] ? 1 : 2;
            if (dep[i] != d || ist[i] != st) return fail("probe", order, ntx, i);
            ext += st == 0;
            if (st == 2 && b_in == CVR_NONE) b_in = i;
        }
        if (mst[t]) o = CVR_EMPTY;
        else if (id[t] != claimed[t]) o = CVR_ID_MISMATCH;
        else {
            for (uint32_t i = tsb[t]; i < tsb[t + 1] && bad == CVN_NO_SIG; i++)
                if (spre[i] || !((bm[i >> 6] >> (i & 63)) & 1)) {
                    bad = i;
                    o = spre[i] == 2 || (spre[i] == 0 && sst[i] == 1) ? CVR_BAD_KEY : CVR_TX_INVALID;
                }
            if (bad == CVN_NO_SIG) {
                if (tsb[t] == tsb[t + 1]) o = CVR_TX_INVALID;
                else if (ck[t] == 3) o = CVR_MALFORMED;
                else if (ck[t] == 2) o = CVR_SIGNATURES_MISSING;
            }
        }
        pre[t] = o;
        if (o == CVR_OK && b_in != CVR_NONE) o = CVR_BAD_INPUT;
        if (outcome[t] != o || fb[t] != bad || bin[t] != (o == CVR_BAD_INPUT ? b_in : CVR_NONE)) return fail("gate", order, ntx, t);
        if ((o == CVR_EMPTY || o == CVR_ID_MISMATCH) && badid == CVR_NONE) badid = t;
        if (count[claimed[t]] > 1 && dup == CVR_NONE) dup = t;
    }
    if (graph[CVR_G_EXTERNAL] != ext) return fail("external", order, ntx, ext);
    const uint32_t status = badid != CVR_NONE ? CVR_GS_BAD_ID : dup != CVR_NONE ? CVR_GS_DUPLICATE_ID : CVR_GS_OK;
    if (graph[CVR_G_STATUS] != status || graph[CVR_G_WHICH] != (badid != CVR_NONE ? badid : dup))
        return fail("status", order, ntx, graph[CVR_G_WHICH]);
    uint32_t n_pass = 0, cls = CVR_NONE, stx = CVR_NONE, sin = CVR_NONE;
    if (status != CVR_GS_OK) {
        for (uint32_t t = 0; t < ntx; t++)
            if (ord[t] != 0) return fail("order not zero", order, ntx, t);
    } else {
        Model m{ntx, claimed, tib, hash, {}, {}, {}};
        m.sort();
        if (m.result.size() != ntx) return fail("model", order, ntx, 0);
        for (uint32_t p = 0; p < ntx; p++)
            if (ord[p] != m.result[p]) return fail("order", order, ntx, p);
        std::set<Id> recorded;
        n_pass = ntx;
        for (uint32_t p = 0; p < ntx && cls == CVR_NONE; p++) {
            const uint32_t t = ord[p];
            if (pre[t] != CVR_OK) cls = pre[t], stx = t;
            for (uint32_t i = tib[t]; i < tib[t + 1] && cls == CVR_NONE; i++) {
                if (!first.count(hash[i])) continue;
                if (!recorded.count(hash[i])) cls = CVR_UNRESOLVED, stx = t, sin = i;
                else if (ist[i] == 2) cls = CVR_BAD_INPUT, stx = t, sin = i;
            }
            if (cls == CVR_NONE) recorded.insert(claimed[t]);
            else n_pass = p;
        }
    }
    if (graph[CVR_G_N_PASS] != n_pass || graph[CVR_G_STOP_CLASS] != cls || graph[CVR_G_STOP_TX] != stx ||
        graph[CVR_G_STOP_INPUT] != sin)
        return fail("walk", order, ntx, graph[CVR_G_STOP_TX]);
    if (tiny && hrs_slots((ntx + 2) / 2) - ntx < 8 && ntx > 8 && graph[CVR_G_MAXPROBE] < 3)
        return fail("no chain in a nearly full table", order, ntx, 0);
    return 0;
}

}  // namespace

int main() {
    unsigned batches = 0;
    const uint32_t sizes[] = {1, 2, 3, 63, 64, 65, 127, 130, 257, 1020, 1025, 1500};
    for (int order = 0; order < 5; order++)
        for (uint32_t ntx : sizes)
            for (int tiny = 0; tiny < 2; tiny++)
                for (int clean = 0; clean < 2; clean++) {
                    if (one_batch(ntx, order, tiny != 0, clean != 0)) return 1;
                    batches++;
                }
    // a chain of 2^20 transactions, each spending the one before it: the reference's visit() would recurse that deep
    {
        const uint32_t n = 1u << 20;
        std::vector<uint32_t> tib(n + 1), dep(n), ord(n), graph(CVR_G_WORDS), bin(n, CVR_NONE);
        std::vector<uint8_t> ist(n, CVR_IN_OK), outcome(n, CVR_OK);
        for (uint32_t t = 0; t <= n; t++) tib[t] = t;
        for (uint32_t t = 0; t < n; t++) dep[t] = t ? t - 1 : CVR_NONE;
        cvr_order(n, tib.data(), dep.data(), ord.data());
        cvr_walk(n, tib.data(), dep.data(), ist.data(), outcome.data(), bin.data(), ord.data(), graph.data());
        for (uint32_t p = 0; p < n; p++)
            if (ord[p] != p) return fail("long chain", 0, n, p);
        if (graph[CVR_G_N_PASS] != n) return fail("long chain walk", 0, n, graph[CVR_G_N_PASS]);
        batches++;
    }
    printf("ok %u\n", batches);
    return 0;
}
