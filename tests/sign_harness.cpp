// sign_harness.cpp — TEST INFRASTRUCTURE: the fixed-key signing procedures of corda_amd/csrc/cv_verify.h
// (cv_key_expand, ge_scalarmult_base_w16, cv_sign_keyed_one; all __host__ __device__) on the CPU, for
// tests/test_sign_keyed_cpu.py, which builds this file into tests/_build/libcvsign.so.
//
// The CV_BW16 rows (4 x 32,769 entries x 128 B) are allocated whole but filled on demand: before a scalar
// multiplication the harness recodes the scalar as the procedure will and builds the (at most 16) entries
// it is about to read (cv_bw16_entry below: the arithmetic of the device's table kernel, on the host).
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../corda_amd/csrc/cv_verify.h"

static void words_from_bytes(uint32_t *w, const uint8_t *b, int nwords) {
    for (int i = 0; i < nwords; i++) memcpy(&w[i], b + 4 * i, 4);
}
static void bytes_from_words(uint8_t *b, const uint32_t *w, int nwords) {
    for (int i = 0; i < nwords; i++) memcpy(b + 4 * i, &w[i], 4);
}

// One CV_BW16 entry, k * 2^(64 row) * B as an affine precomp (y+x, y-x, 2dxy), canonical limbs: the arithmetic of
// cv_bw16_init_kernel (cv_k_hs.hip), one entry at a time with the same per-lane procedures.
static void cv_bw16_entry(uint32_t *o, uint32_t row, uint32_t k, const uint32_t *btab) {
    uint32_t sc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    sc[2 * row] = k;                       // k * 2^(64 row)
    ge_p3 P;
    ge_scalarmult_base(P, sc, btab);
    fe zi, x, y, xy, d2, f[3];
    fe_invert(zi, P.Z);
    fe_mul(x, P.X, zi);
    fe_mul(y, P.Y, zi);
    fe_add(f[0], y, x);
    fe_sub<2>(f[1], y, x);
    fe_mul(xy, x, y);
    fe_const_d2(d2);
    fe_mul(f[2], xy, d2);
    for (int c = 0; c < 3; c++) {
        uint32_t w[8];
        fe_to_words(w, f[c]);
        fe canon;
        fe_from_words(canon, w);
        fe_store(o + 10 * c, canon);
    }
    o[30] = o[31] = 0;
}

static uint32_t *g_bw16;                   // CV_BW16_ROWS * CV_BW16_ROW words, 16-B aligned, zero until built
static std::vector<uint8_t> g_built;       // one flag per entry
static size_t g_nbuilt;

// build the entries [k]B will read for this scalar (k < 2^253)
static const uint32_t *bw16_for(const uint32_t k[8]) {
    if (!g_bw16) {
        g_bw16 = static_cast<uint32_t *>(aligned_alloc(16, (size_t)CV_BW16_ROWS * CV_BW16_ROW * 4));
        memset(g_bw16, 0, (size_t)CV_BW16_ROWS * CV_BW16_ROW * 4);
        g_built.assign((size_t)CV_BW16_ROWS * CV_BW16_ENTRIES, 0);
    }
    uint32_t kd[8];
    digits65536_pairs(kd, k);
    for (int i = 0; i < 16; i++) {          // digit i: row i / 4, column i % 4
        const uint32_t word = kd[i & 7];
        const int d = i < 8 ? (int)(int16_t)(word & 0xffffu) : (int)word >> 16;
        const uint32_t m = (uint32_t)(d < 0 ? -d : d), row = (uint32_t)i / 4;
        const size_t t = (size_t)row * CV_BW16_ENTRIES + m;
        if (!g_built[t]) {
            cv_bw16_entry(g_bw16 + t * CV_BTAB_STRIDE, row, m, CV_BTAB_H);
            g_built[t] = 1;
            g_nbuilt++;
        }
    }
    return g_bw16;
}

extern "C" {

// entries of the CV_BW16 table built so far (the tests check that it stays a small part of the table)
size_t cvs_bw16_built(void) { return g_nbuilt; }

// seed -> a, prefix, abyte (32 bytes each)
void cvs_key_expand(const uint8_t *seed, uint8_t *a, uint8_t *prefix, uint8_t *abyte) {
    uint32_t sd[8], aw[8], pw[8], bw[8];
    words_from_bytes(sd, seed, 8);
    cv_key_expand(sd, aw, pw, bw, CV_BTAB_H);
    bytes_from_words(a, aw, 8);
    bytes_from_words(prefix, pw, 8);
    bytes_from_words(abyte, bw, 8);
}

// enc([k]B) for a 32-byte little-endian scalar k < 2^253
void cvs_scalarmult_base_w16(const uint8_t *k, uint8_t *enc) {
    uint32_t kw[8], ew[8];
    words_from_bytes(kw, k, 8);
    ge_p3 R;
    ge_scalarmult_base_w16(R, kw, bw16_for(kw));
    ge_p3_encode(ew, R);
    bytes_from_words(enc, ew, 8);
}

// the signature of msg under an expanded key (a, prefix, abyte as cvs_key_expand returns them)
void cvs_sign_keyed(const uint8_t *a, const uint8_t *prefix, const uint8_t *abyte, const uint8_t *msg, uint32_t mlen,
                    uint8_t *sig) {
    uint32_t aw[8], pw[8], bw[8], sg[16];
    words_from_bytes(aw, a, 8);
    words_from_bytes(pw, prefix, 8);
    words_from_bytes(bw, abyte, 8);
    // r, as cv_sign_keyed_one derives it, to build the entries [r]B reads
    uint32_t pre[16], rd[16], r[8];
    for (int q = 0; q < 8; q++) { pre[q] = pw[q]; pre[8 + q] = 0; }
    sha512_pre_msg(rd, pre, 32, msg, mlen);
    sc_reduce512(r, rd);
    cv_sign_keyed_one(bw16_for(r), aw, pw, bw, msg, mlen, sg);
    bytes_from_words(sig, sg, 16);
}

}  // extern "C"
