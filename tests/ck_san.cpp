// ck_san.cpp — TEST INFRASTRUCTURE: the missing-signers core (corda_amd/csrc/cv_ck.h through tests/ck_harness.cpp) as a
// stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_ck_cpu.py builds and runs it as a
// subprocess).  Random forests — trees, DAGs with shared children, negative and wrapping weights, duplicate signers —
// and forests whose child arrays are hostile (indices and ranges anywhere in 32 bits) against a sequential
// restatement, with every array in a heap block of exactly its size so a read outside it is an ASan report; then wide
// shapes (signer and Leaf counts around CV_CK_TILE and a 300 x 300 outlier).  Prints "ok <forests>" or the first difference.
#include <cstdio>

#include "ck_harness.cpp"

namespace {

struct Rng {
    uint64_t x;
    uint32_t next() {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(x >> 32);
    }
    uint32_t below(uint32_t n) { return n ? next() % n : 0; }
};

struct Forest {
    std::vector<uint8_t> kind, leaf_key, sig_key, allowed;
    std::vector<int32_t> threshold, weight;
    std::vector<uint32_t> child_begin{0}, child, req_begin{0}, tx_req_begin{0}, tx_sig_begin{0};
    std::vector<uint64_t> bitmap;
    bool with_bitmap = false;
    uint32_t ntx() const { return (uint32_t)tx_req_begin.size() - 1; }
    uint32_t nreq() const { return (uint32_t)req_begin.size() - 1; }
    uint32_t nnodes() const { return (uint32_t)kind.size(); }
    uint32_t nsig() const { return (uint32_t)sig_key.size() / 32; }
};

void put_key(std::vector<uint8_t> &v, uint32_t id) {
    // 32 bytes from a small id: keys of ids that agree modulo 7 share their first 8 bytes
    for (int i = 0; i < 32; i++) v.push_back((uint8_t)(i < 8 ? (id % 7) * 31 + i : id * 131 + i * 17 + (id >> 3)));
}

// a sequential restatement over the flat arrays: the requirement's nodes in order, everything checked
uint8_t ref_requirement(const Forest &f, uint32_t r, uint32_t sb, uint32_t se) {
    const uint32_t rb = f.req_begin[r], re = f.req_begin[r + 1];
    if (rb >= re) return 2;
    std::vector<uint8_t> flag(re - rb, 0);
    bool bad = false;
    for (uint32_t k = rb; k < re; k++) {
        if (f.kind[k] == 0) {
            for (uint32_t s = sb; s < se; s++)
                if (!memcmp(&f.leaf_key[32 * (size_t)k], &f.sig_key[32 * (size_t)s], 32)) flag[k - rb] = 1;
        } else if (f.kind[k] == 1) {
            const uint64_t cb = f.child_begin[k], ce = f.child_begin[k + 1];
            if (cb > ce || ce > f.child.size()) {
                bad = true;
                continue;
            }
            int64_t sum = 0;
            bool ok = true;
            for (uint64_t j = cb; j < ce && ok; j++) {
                const uint32_t c = f.child[j];
                if (c < rb || c >= k) ok = false;
                else if (flag[c - rb]) sum += f.weight[j];
            }
            if (!ok) {
                bad = true;
                continue;
            }
            // Kotlin's Int: the exact sum reduced to 32 bits, two's complement
            const int64_t wrapped = ((sum % 4294967296ll) + 4294967296ll) % 4294967296ll;
            const int64_t as_int = wrapped >= 2147483648ll ? wrapped - 4294967296ll : wrapped;
            flag[k - rb] = as_int >= (int64_t)f.threshold[k];
        } else {
            bad = true;
        }
    }
    return bad ? 2 : flag[re - rb - 1] ? 0 : 1;
}

void reference(const Forest &f, std::vector<uint8_t> &rm, std::vector<uint8_t> &st) {
    rm.assign(f.nreq(), 0);
    st.assign(f.ntx(), 0);
    for (uint32_t t = 0; t < f.ntx(); t++) {
        const uint32_t sb = f.tx_sig_begin[t], se = f.tx_sig_begin[t + 1];
        bool mal = false, need = false, badsig = sb == se;
        for (uint32_t r = f.tx_req_begin[t]; r < f.tx_req_begin[t + 1]; r++) {
            rm[r] = ref_requirement(f, r, sb, se);
            mal |= rm[r] == 2;
            need |= rm[r] == 1 && !f.allowed[r];
        }
        if (f.with_bitmap)
            for (uint32_t s = sb; s < se; s++) badsig |= !((f.bitmap[s / 64] >> (s % 64)) & 1);
        st[t] = mal ? 3 : badsig ? 1 : need ? 2 : 0;
    }
}

// one requirement of up to `maxn` nodes: Leaves and Nodes over earlier nodes (shared children and repeats happen)
void add_requirement(Forest &f, Rng &g, uint32_t maxn, uint32_t key_pool, int hostile) {
    const uint32_t rb = f.nnodes(), n = 1 + g.below(maxn);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t k = rb + i;
        const bool node = i > 0 && g.below(3) == 0;
        f.kind.push_back(node ? 1 : 0);
        if (hostile && g.below(40) == 0) f.kind.back() = (uint8_t)(2 + g.below(254));
        if (node) {
            for (int q = 0; q < 32; q++) f.leaf_key.push_back(0);
            const uint32_t nc = g.below(5);
            for (uint32_t j = 0; j < nc; j++) {
                uint32_t c = rb + g.below(k - rb);
                if (hostile && g.below(12) == 0) c = g.below(4) ? g.next() : (g.below(2) ? k : rb - 1);
                f.child.push_back(c);
                const uint32_t kindw = g.below(8);
                const int32_t w = kindw == 0 ? (int32_t)g.next() : kindw == 1 ? -(int32_t)g.below(5) : kindw == 2 ? (1 << 30) : (int32_t)(1 + g.below(4));
                f.weight.push_back(w);
            }
            const uint32_t tk = g.below(6);
            f.threshold.push_back(tk == 0 ? (int32_t)g.next() : tk == 1 ? 0 : tk == 2 ? -1 : (int32_t)(1 + g.below(nc + 1)));
        } else {
            put_key(f.leaf_key, g.below(key_pool));
            f.threshold.push_back(0);
        }
        f.child_begin.push_back((uint32_t)f.child.size());
        if (hostile && g.below(25) == 0) f.child_begin.back() = g.below(3) ? g.next() : (uint32_t)f.child.size() + 1 + g.below(3);
    }
    f.req_begin.push_back(f.nnodes());
    f.allowed.push_back(g.below(4) == 0);
}

Forest random_forest(Rng &g, int hostile) {
    Forest f;
    const uint32_t ntx = 1 + g.below(70), key_pool = 3 + g.below(40);
    for (uint32_t t = 0; t < ntx; t++) {
        const uint32_t nr = g.below(5);
        for (uint32_t r = 0; r < nr; r++) {
            if (hostile && g.below(30) == 0) {                     // an empty requirement
                f.req_begin.push_back(f.nnodes());
                f.allowed.push_back(0);
            } else {
                add_requirement(f, g, g.below(6) ? 6 : 40, key_pool, hostile);
            }
        }
        f.tx_req_begin.push_back(f.nreq());
        const uint32_t ns = g.below(8) ? g.below(6) : g.below(150);
        for (uint32_t s = 0; s < ns; s++) put_key(f.sig_key, g.below(key_pool));
        f.tx_sig_begin.push_back(f.nsig());
    }
    // the host form's contract: child_begin ends at nchild
    f.child_begin.back() = (uint32_t)f.child.size();
    f.with_bitmap = g.below(2);
    f.bitmap.assign((f.nsig() + 63) / 64, 0);
    for (auto &w : f.bitmap) w = ((uint64_t)g.next() << 32 | g.next()) | ((uint64_t)g.next() << 32 | g.next()) | ((uint64_t)g.next() << 32 | g.next());
    return f;
}

// Leaf counts and signer counts around the tile, the match in the last key of the last tile, the first key, nowhere
Forest wide_forest(uint32_t nl, uint32_t ns, int where) {
    Forest f;
    for (uint32_t i = 0; i < nl; i++) {
        f.kind.push_back(0);
        put_key(f.leaf_key, 1000 + i);
        f.threshold.push_back(0);
        f.child_begin.push_back(0);
    }
    f.kind.push_back(1);
    for (int q = 0; q < 32; q++) f.leaf_key.push_back(0);
    f.threshold.push_back(1);
    for (uint32_t i = 0; i < nl; i++) f.child.push_back(i), f.weight.push_back(1);
    f.child_begin.push_back(nl);
    f.req_begin.push_back(nl + 1);
    f.allowed.push_back(0);
    f.tx_req_begin.push_back(1);
    for (uint32_t s = 0; s < ns; s++) put_key(f.sig_key, (where == 0 && s == ns - 1) || (where == 1 && s == 0) ? 1000 + nl - 1 : 5000 + s);
    f.tx_sig_begin.push_back(ns);
    return f;
}

template <class T> T *exact(const std::vector<T> &v, std::vector<T *> &keep) {
    // a heap block of exactly the array's size (one element when it is empty, which nothing may read meaningfully)
    T *p = static_cast<T *>(malloc(v.size() ? v.size() * sizeof(T) : sizeof(T)));
    if (v.size()) memcpy(p, v.data(), v.size() * sizeof(T));
    else memset(p, 0x77, sizeof(T));
    keep.push_back(p);
    return p;
}

int check(const Forest &f, const char *what, uint64_t id) {
    std::vector<uint8_t> want_rm, want_st;
    reference(f, want_rm, want_st);
    std::vector<uint8_t *> k8;
    std::vector<int32_t *> ki;
    std::vector<uint32_t *> ku;
    std::vector<uint64_t *> kq;
    const uint8_t *kind = exact(f.kind, k8), *key = exact(f.leaf_key, k8), *sig = exact(f.sig_key, k8), *al = exact(f.allowed, k8);
    const int32_t *thr = exact(f.threshold, ki), *w = exact(f.weight, ki);
    const uint32_t *cb = exact(f.child_begin, ku), *ch = exact(f.child, ku), *rb = exact(f.req_begin, ku);
    const uint32_t *trb = exact(f.tx_req_begin, ku), *tsb = exact(f.tx_sig_begin, ku);
    const uint64_t *bm = f.with_bitmap ? exact(f.bitmap, kq) : nullptr;
    int rc = 0;
    const uint32_t wide_mins[3] = {0u, 1u, 0xffffffffu};
    for (uint32_t wm : wide_mins)
        for (int order = 0; order < 3 && !rc; order++) {
            std::vector<uint8_t *> ko;
            uint8_t *rm = exact(std::vector<uint8_t>(f.nreq(), 0xEE), ko), *st = exact(std::vector<uint8_t>(f.ntx(), 0xEE), ko);
            const int64_t wide = hck_run(f.ntx(), f.nreq(), f.nnodes(), (uint32_t)f.child.size(), f.nsig(), kind, key, thr, cb, ch, w,
                                         rb, trb, sig, tsb, al, bm, wm, order, rm, st);
            if (wide < 0 || (wm == 1 && wide != (int64_t)f.ntx()) || (wm == 0xffffffffu && wide != 0)) rc = 1;
            if (f.nreq() && memcmp(rm, want_rm.data(), f.nreq())) rc = 1;
            if (memcmp(st, want_st.data(), f.ntx())) rc = 1;
            if (rc) printf("DIFFERENT: %s %llu wide_min %u order %d\n", what, (unsigned long long)id, wm, order);
            for (auto p : ko) free(p);
        }
    for (auto p : k8) free(p);
    for (auto p : ki) free(p);
    for (auto p : ku) free(p);
    for (auto p : kq) free(p);
    return rc;
}

}  // namespace

int main() {
    Rng g{0x243F6A8885A308D3ull};
    uint64_t n = 0;
    for (int i = 0; i < 300; i++, n++)
        if (check(random_forest(g, 0), "forest", i)) return 1;
    for (int i = 0; i < 300; i++, n++)
        if (check(random_forest(g, 1), "hostile forest", i)) return 1;
    const uint32_t T = CV_CK_TILE, leaves[4] = {63, 64, 65, 129}, signers[4] = {T - 1, T, T + 1, 2 * T + 1};
    for (uint32_t nl : leaves)
        for (uint32_t ns : signers)
            for (int where = 0; where < 3; where++, n++)
                if (check(wide_forest(nl, ns, where), "wide", nl * 1000 + ns)) return 1;
    if (check(wide_forest(300, 300, 0), "outlier", 0)) return 1;
    printf("ok %llu\n", (unsigned long long)(n + 1));
    return 0;
}
