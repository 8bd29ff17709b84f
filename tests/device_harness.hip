// device_harness.hip — TEST INFRASTRUCTURE: the product's device code (corda_amd/csrc/cv_hsquad.h, which pulls in
// cv_quad.h and cv_verify.h) behind small test kernels, so the forms that exist only on the GPU — the
// v_mad_u64_u32 columns of cv_madc.h, the hardware reciprocal in cv_qdiv, the DPP quad formulas, the device
// variants in cv_sha.h — can be compared value by value with big-integer references
// (tests/test_gpu_device_logic.py).  Built by that module's fixture into tests/_build/libcvdev.so with the
// product's kernel flags.
//
// Every entry point is extern "C", takes host pointers, does its own hipMalloc / hipMemcpy / launch /
// hipDeviceSynchronize / copy back / hipFree, and returns the first non-zero hipError_t (0 = success; -1 = a
// bad argument).  One item per lane; the quad kernels run four lanes per point (lane r = coordinate r of
// (X, Y, Z, T)) in whole waves, so their item counts must be multiples of 16 points.
#include <cstdint>
#include <cstring>

#include "../corda_amd/csrc/cv_hsquad.h"

#define CVD_BLOCK 64
// Five translation units from this one file, compiled side by side (the whole file in one took 78 s):
// -DCVD_PART=1 field, scalars and hashes; 2 the quad kernels in the ILP field forms (SEQ = false) and the bit
// packing; 3 the quad kernels in the sequential-carry forms (SEQ = true, what production instantiates); 4 decode
// and tables with LAT = false; 5 the same with LAT = true.
#if !defined(CVD_PART) || CVD_PART < 1 || CVD_PART > 5
#error "compile with -DCVD_PART=1 .. 5"
#endif
#define CVD_HAS(part) ((part) == 2 ? (CVD_PART == 2 || CVD_PART == 3) : (part) == 4 ? CVD_PART >= 4 : CVD_PART == (part))
#define CVD_SEQ (CVD_PART == 3)
#define CVD_LAT (CVD_PART == 5)

namespace {

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

#define CVD_TRY(x)                      \
    do {                                \
        const hipError_t e_ = (x);      \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)

// in: n x inw words, out: n x outw words (zeroed before the launch), aux: optional read-only bytes,
// scratch_words: optional zeroed device words.  lanes = threads launched (a multiple of CVD_BLOCK for the quad kernels).
template <typename K>
int run(K kernel, uint32_t n, uint32_t lanes, const uint32_t *in, size_t inw, uint32_t *out, size_t outw,
        const void *aux = nullptr, size_t aux_bytes = 0, size_t scratch_words = 0) {
    if (n == 0 || lanes == 0 || lanes > (1u << 20)) return -1;
    DevBuf din, dout, daux, dscr;
    CVD_TRY(hipMalloc(&din.p, (size_t)n * inw * 4));
    CVD_TRY(hipMalloc(&dout.p, (size_t)n * outw * 4));
    CVD_TRY(hipMemcpy(din.p, in, (size_t)n * inw * 4, hipMemcpyHostToDevice));
    CVD_TRY(hipMemset(dout.p, 0, (size_t)n * outw * 4));
    if (aux_bytes) {
        CVD_TRY(hipMalloc(&daux.p, aux_bytes));
        CVD_TRY(hipMemcpy(daux.p, aux, aux_bytes, hipMemcpyHostToDevice));
    }
    if (scratch_words) {
        CVD_TRY(hipMalloc(&dscr.p, scratch_words * 4));
        CVD_TRY(hipMemset(dscr.p, 0, scratch_words * 4));
    }
    hipLaunchKernelGGL(kernel, dim3((lanes + CVD_BLOCK - 1) / CVD_BLOCK), dim3(CVD_BLOCK), 0, 0, n,
                       static_cast<const uint32_t *>(din.p), static_cast<uint32_t *>(dout.p),
                       static_cast<const uint8_t *>(daux.p), static_cast<uint32_t *>(dscr.p));
    CVD_TRY(hipGetLastError());
    CVD_TRY(hipDeviceSynchronize());
    CVD_TRY(hipMemcpy(out, dout.p, (size_t)n * outw * 4, hipMemcpyDeviceToHost));
    return 0;
}

#define CVD_ARGS uint32_t n, const uint32_t *__restrict__ in, uint32_t *__restrict__ out, const uint8_t *aux, uint32_t *scr
#define CVD_LANE(INW, OUTW)                                              \
    const uint32_t i = blockIdx.x * CVD_BLOCK + threadIdx.x;             \
    if (i >= n) return;                                                  \
    const uint32_t *x = in + (size_t)i * (INW);                          \
    uint32_t *y = out + (size_t)i * (OUTW);                              \
    (void)aux; (void)scr

__device__ __forceinline__ void ld(fe &f, const uint32_t *p) { fe_load(f, p); }
__device__ __forceinline__ void st(uint32_t *p, const fe &f) { fe_store(p, f); }

#if CVD_HAS(1)
// ---------------------------------------------------------------- field
// FORM 0 fe_mul, 1 fe_mul_ilp: in f | g, out h
template <int FORM> __global__ void k_mul(CVD_ARGS) {
    CVD_LANE(20, 10);
    fe f, g, h;
    ld(f, x); ld(g, x + 10);
    if constexpr (FORM == 0) fe_mul(h, f, g); else fe_mul_ilp(h, f, g);
    st(y, h);
}
// fe_mul_n<N>: in f[0..N) | g[0..N), out h[0..N)
template <int N> __global__ void k_muln(CVD_ARGS) {
    CVD_LANE(20 * N, 10 * N);
    fe f[N], g[N], h[N];
    for (int m = 0; m < N; m++) { ld(f[m], x + 10 * m); ld(g[m], x + 10 * N + 10 * m); }
    fe_mul_n<N>(h, f, g);
    for (int m = 0; m < N; m++) st(y + 10 * m, h[m]);
}
// FORM 0 fe_sq, 1 fe_sq2, 2 fe_sq_rt(flag), 3 fe_sq_ilp(flag): in f | flag, out h
template <int FORM> __global__ void k_sq(CVD_ARGS) {
    CVD_LANE(11, 10);
    fe f, h;
    ld(f, x);
    const bool dbl = x[10] != 0;
    if constexpr (FORM == 0) fe_sq(h, f);
    else if constexpr (FORM == 1) fe_sq2(h, f);
    else if constexpr (FORM == 2) fe_sq_rt(h, f, dbl);
    else fe_sq_ilp(h, f, dbl);
    st(y, h);
}
template <int N, unsigned DBL> __global__ void k_sqn(CVD_ARGS) {
    CVD_LANE(10 * N, 10 * N);
    fe f[N], h[N];
    for (int m = 0; m < N; m++) ld(f[m], x + 10 * m);
    fe_sq_n<N, DBL>(h, f);
    for (int m = 0; m < N; m++) st(y + 10 * m, h[m]);
}
// FORM 0 fe_sub<2>, 1 fe_sub<3>, 2 fe_sub<4>, 3 fe_sub_carry_even<3>: in f | g, out h
template <int FORM> __global__ void k_sub(CVD_ARGS) {
    CVD_LANE(20, 10);
    fe f, g, h;
    ld(f, x); ld(g, x + 10);
    if constexpr (FORM == 0) fe_sub<2>(h, f, g);
    else if constexpr (FORM == 1) fe_sub<3>(h, f, g);
    else if constexpr (FORM == 2) fe_sub<4>(h, f, g);
    else fe_sub_carry_even<3>(h, f, g);
    st(y, h);
}
// FORM 0 fe_carry, 1 fe_carry_even, 2 fe_neg, 3 fe_invert<false>, 4 fe_invert<true>, 5 fe_pow22523<false>,
// 6 fe_pow22523<true>: in f, out h
template <int FORM> __global__ void k_un(CVD_ARGS) {
    CVD_LANE(10, 10);
    fe f, h;
    ld(f, x);
    if constexpr (FORM == 0) fe_carry(h, f);
    else if constexpr (FORM == 1) { h = f; fe_carry_even(h); }
    else if constexpr (FORM == 2) fe_neg(h, f);
    else if constexpr (FORM == 3) fe_invert<false>(h, f);
    else if constexpr (FORM == 4) fe_invert<true>(h, f);
    else if constexpr (FORM == 5) fe_pow22523<false>(h, f);
    else fe_pow22523<true>(h, f);
    st(y, h);
}
// in: 8 words | 10 limbs; out: fe_from_words(words) limbs (10) | fe_to_words(limbs) (8)
__global__ void k_words(CVD_ARGS) {
    CVD_LANE(18, 18);
    uint32_t w[8], o[8];
    for (int q = 0; q < 8; q++) w[q] = x[q];
    fe f, g;
    fe_from_words(f, w);
    st(y, f);
    ld(g, x + 8);
    fe_to_words(o, g);
    for (int q = 0; q < 8; q++) y[10 + q] = o[q];
}

// ---------------------------------------------------------------- scalars
__global__ void k_sc_reduce(CVD_ARGS) {
    CVD_LANE(16, 8);
    uint32_t a[16], o[8];
    for (int q = 0; q < 16; q++) a[q] = x[q];
    sc_reduce512(o, a);
    for (int q = 0; q < 8; q++) y[q] = o[q];
}
__global__ void k_sc_muladd(CVD_ARGS) {
    CVD_LANE(24, 8);
    uint32_t a[8], b[8], c[8], o[8];
    for (int q = 0; q < 8; q++) { a[q] = x[q]; b[q] = x[8 + q]; c[q] = x[16 + q]; }
    sc_muladd(o, a, b, c);
    for (int q = 0; q < 8; q++) y[q] = o[q];
}
// one quotient step of sc_halfsize's exact loop, as the host harness's cvh_exact_step: in r0 | r1, out q | r0 - q r1
__global__ void k_exact_step(CVD_ARGS) {
    CVD_LANE(16, 9);
    uint32_t r0[8], r1[8];
    for (int q = 0; q < 8; q++) { r0[q] = x[q]; r1[q] = x[8 + q]; }
    const uint32_t q = cv_exact_quotient(r0, r1);
    cv_submul8(r0, r1, q);
    y[0] = q;
    for (int k = 0; k < 8; k++) y[1 + k] = r0[k];
}
// in h | s, out u | |v| | w | v_neg | nwin | ok
__global__ void k_halfsize(CVD_ARGS) {
    CVD_LANE(16, 27);
    uint32_t h[8], s[8], u[8], v[8], w[8];
    for (int q = 0; q < 8; q++) { h[q] = x[q]; s[q] = x[8 + q]; }
    bool neg = false;
    int nw = 0;
    const bool ok = sc_halfsize(u, v, neg, nw, w, h, s);
    for (int q = 0; q < 8; q++) { y[q] = u[q]; y[8 + q] = v[q]; y[16 + q] = w[q]; }
    y[24] = neg ? 1 : 0;
    y[25] = (uint32_t)nw;
    y[26] = ok ? 1 : 0;
}
// cv_hs_scalars<B16, W16>: in h | s, out the CV_HS_DIGWORDS words at stride 1 (words the form leaves alone stay 0)
template <bool B16, bool W16> __global__ void k_hs_scalars(CVD_ARGS) {
    CVD_LANE(16, CV_HS_DIGWORDS);
    uint32_t hs[CV_HS_WORDS];
    for (int q = 0; q < 16; q++) hs[q] = x[q];
    cv_hs_scalars<B16, W16>(hs, y, 1);
}

// ---------------------------------------------------------------- hashes
// in: pre (16 words) | npre (32 or 64) | message offset in aux | message length; out: SHA-512(pre[:npre] || msg) as
// sha512_pre_msg leaves it (16 words) | sha256_bytes(msg) (8 words)
__global__ void k_sha(CVD_ARGS) {
    CVD_LANE(19, 24);
    uint32_t pre[16], o[16], o2[8];
    for (int q = 0; q < 16; q++) pre[q] = x[q];
    sha512_pre_msg(o, pre, (int)x[16], aux + x[17], x[18]);
    for (int q = 0; q < 16; q++) y[q] = o[q];
    sha256_bytes(o2, aux + x[17], x[18]);
    for (int q = 0; q < 8; q++) y[16 + q] = o2[q];
}

#endif  // part 1
#if CVD_HAS(4)
// ---------------------------------------------------------------- decode and tables
__device__ __forceinline__ void st_p3(uint32_t *p, const ge_p3 &P) {
    st(p, P.X); st(p + 10, P.Y); st(p + 20, P.Z); st(p + 30, P.T);
}
// in: 8 words; out: ok | ge_p2_encode of the point (8) | cv_r_canonical | ge_abyte_from_key (8) | X Y Z T limbs (40)
template <bool LAT> __global__ void k_decode(CVD_ARGS) {
    CVD_LANE(8, 58);
    uint32_t w[8], e[8];
    for (int q = 0; q < 8; q++) w[q] = x[q];
    ge_p3 A;
    y[0] = ge_decode_0_1_0<LAT>(A, w) ? 1 : 0;
    ge_p3_encode(e, A);
    for (int q = 0; q < 8; q++) y[1 + q] = e[q];
    y[9] = cv_r_canonical(w) ? 1 : 0;
    ge_abyte_from_key(e, w);
    for (int q = 0; q < 8; q++) y[10 + q] = e[q];
    st_p3(y + 18, A);
}
// in: 8 + 8 words; out per encoding: ok | encode (8) | X Y Z T limbs (40)
template <bool LAT> __global__ void k_decode2(CVD_ARGS) {
    CVD_LANE(16, 98);
    uint32_t w0[8], w1[8], e[8];
    for (int q = 0; q < 8; q++) { w0[q] = x[q]; w1[q] = x[8 + q]; }
    ge_p3 A[2];
    bool ok[2];
    ge_decode2_0_1_0<LAT>(A, ok, w0, w1);
    for (int k = 0; k < 2; k++) {
        y[49 * k] = ok[k] ? 1 : 0;
        ge_p3_encode(e, A[k]);
        for (int q = 0; q < 8; q++) y[49 * k + 1 + q] = e[q];
        st_p3(y + 49 * k + 9, A[k]);
    }
}
// cv_hs_point_one<LAT>: in 8 words | is_r | half + 1 (0, 1, 2); out the 9-entry table (360 words) | flag | pad 3
template <bool LAT> __global__ void k_point_one(CVD_ARGS) {
    CVD_LANE(10, 364);
    uint32_t w[8];
    for (int q = 0; q < 8; q++) w[q] = x[q];
    y[360] = cv_hs_point_one<LAT>(w, x[8] != 0, y, (int)x[9] - 1) ? 1 : 0;
}
// cv_hs_points<LAT>: in key | R; out tabA (360) | tabR (360) | key_ok | ok_out | pad 2
template <bool LAT> __global__ void k_points(CVD_ARGS) {
    CVD_LANE(16, 724);
    uint32_t aw[8], rw[8];
    for (int q = 0; q < 8; q++) { aw[q] = x[q]; rw[q] = x[8 + q]; }
    bool ok = false;
    y[720] = cv_hs_points<LAT>(aw, rw, y, y + 360, ok) ? 1 : 0;
    y[721] = ok ? 1 : 0;
}

#endif  // part 4
#if CVD_HAS(2)
// ---------------------------------------------------------------- quad: four lanes per point
// Whole waves, every lane active (n is a multiple of 16 points: the entry points check it).
#define CVD_QUAD(INW, OUTW)                                              \
    const uint32_t lane = blockIdx.x * CVD_BLOCK + threadIdx.x;          \
    const uint32_t i = lane >> 2;                                        \
    const int r = (int)(lane & 3u);                                      \
    const uint32_t *x = in + (size_t)i * (INW);                          \
    uint32_t *y = out + (size_t)i * (OUTW);                              \
    (void)aux; (void)scr; (void)n

// in X Y Z T, out X Y Z T of 2P
template <bool SEQ> __global__ void k_quad_dbl(CVD_ARGS) {
    CVD_QUAD(40, 40);
    fe P;
    ld(P, x + 10 * r);
    quad_dbl<SEQ>(P, r);
    st(y + 10 * r, P);
}
// The k P table (k = 0..8, cached form) of the point at q, built by the quad's lane 0 into the point's scratch slot
__device__ __forceinline__ const uint32_t *quad_build_table(uint32_t *scr, uint32_t i, const uint32_t *q, int r) {
    uint32_t *tab = scr + (size_t)i * CV_TAB_WORDS;
    if (r == 0) {
        ge_p3 Q;
        ld(Q.X, q); ld(Q.Y, q + 10); ld(Q.Z, q + 20); ld(Q.T, q + 30);
        ge_cached_multiples8(tab, Q);
    }
    __threadfence();
    __syncthreads();
    return tab;
}
// quad_add<SEQ> with its operand from MODE 0 quad_cached_coord, 1 quad_precomp_coord, 2 quad_any_coord over a
// cached table, 3 quad_any_coord over affine rows.
// in: P (40) | Q (40: the table's point, modes 0 and 2) | digit | table word offset | from aux (else CV_BCOMB) |
// stride | ident_row | pad 3;  out: P + digit * (table point)
template <bool SEQ, int MODE> __global__ void k_quad_add(CVD_ARGS) {
    CVD_QUAD(88, 40);
    fe P, q;
    ld(P, x + 10 * r);
    const int d = (int)x[80];
    if constexpr (MODE == 0 || MODE == 2) {
        const uint32_t *tab = quad_build_table(scr, i, x + 40, r);
        if constexpr (MODE == 0) quad_cached_coord(q, tab, d, r); else quad_any_coord(q, tab, false, d, r);
    } else {
        const uint32_t *tab = (x[82] ? reinterpret_cast<const uint32_t *>(aux) : CV_BCOMB) + x[81];
        if constexpr (MODE == 1) quad_precomp_coord(q, tab, (int)x[83], d, r, x[84] != 0);
        else quad_any_coord(q, tab, true, d, r);
    }
    quad_add<SEQ>(P, q, r);
    st(y + 10 * r, P);
}
// in X Y Z T, out the cached form (Y+X, Y-X, Z, 2dT)
template <bool SEQ> __global__ void k_quad_to_cached(CVD_ARGS) {
    CVD_QUAD(40, 40);
    fe P, q;
    ld(P, x + 10 * r);
    quad_to_cached<SEQ>(q, P, r);
    st(y + 10 * r, q);
}
// The tail of cv_tri_hs_straus: sixteen lanes hold four points, one per quad; after the two row rotations every
// quad holds the sum of the four.  (Items are quads here: in / out X Y Z T per quad.)
template <bool SEQ> __global__ void k_tri_sum(CVD_ARGS) {
    CVD_QUAD(40, 40);
    fe P, Q, q;
    ld(P, x + 10 * r);
    fe_dpp_row<0x124>(Q, P);                             // row_ror:4
    quad_to_cached<SEQ>(q, Q, r);
    quad_add<SEQ>(P, q, r);
    fe_dpp_row<0x128>(Q, P);                             // row_ror:8
    quad_to_cached<SEQ>(q, Q, r);
    quad_add<SEQ>(P, q, r);
    st(y + 10 * r, P);
}
// Eight windows of four quad_dbl and one quad_add (digit from the table of Q, quad_cached_coord), the point stored
// after every one of the 40 steps.  in: P (40) | Q (40) | 8 digits; out 40 x (X Y Z T)
#define CVD_CHAIN_WIN 8
template <bool SEQ> __global__ void k_quad_chain(CVD_ARGS) {
    CVD_QUAD(88, 40 * 5 * CVD_CHAIN_WIN);
    fe P, q;
    ld(P, x + 10 * r);
    const uint32_t *tab = quad_build_table(scr, i, x + 40, r);
    int step = 0;
#pragma unroll 1
    for (int win = 0; win < CVD_CHAIN_WIN; win++) {
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
            quad_dbl<SEQ>(P, r);
            st(y + 40 * step++ + 10 * r, P);
        }
        quad_cached_coord(q, tab, (int)x[80 + win], r);
        quad_add<SEQ>(P, q, r);
        st(y + 40 * step++ + 10 * r, P);
    }
}

// ---------------------------------------------------------------- verdict bit packing
// in: a 64-bit ballot mask (2 words); out: cv_quad_ballot_bits(mask) | the tri kernel's four bits (lanes 0, 16, 32,
// 48: the three lines of cv_hs_straus_tri_kernel)
__global__ void k_ballot(CVD_ARGS) {
    CVD_LANE(2, 2);
    const uint64_t m = x[0] | ((uint64_t)x[1] << 32);
    y[0] = cv_quad_ballot_bits(m);
    uint64_t b = m & 0x0001000100010001ull;
    b = (b | (b >> 15)) & 0x0000000300000003ull;
    b = (b | (b >> 30)) & 0xfull;
    y[1] = (uint32_t)b;
}

template <typename K> int quad_run(K kernel, uint32_t n, const uint32_t *in, size_t inw, uint32_t *out, size_t outw,
                                   const void *aux = nullptr, size_t aux_bytes = 0, bool scratch = false) {
    if (n == 0 || n % 16 != 0) return -1;
    return run(kernel, n, 4 * n, in, inw, out, outw, aux, aux_bytes, scratch ? (size_t)n * CV_TAB_WORDS : 0);
}

#endif  // part 2

}  // namespace

// the product's flags hide host symbols (-fvisibility=hidden): the entry points are the exceptions
#pragma GCC visibility push(default)
extern "C" {

#if CVD_HAS(1)
int cvd_fe_mul(int form, uint32_t n, const uint32_t *in, uint32_t *out) {
    switch (form) {
    case 0: return run(k_mul<0>, n, n, in, 20, out, 10);
    case 1: return run(k_mul<1>, n, n, in, 20, out, 10);
    }
    return -1;
}
int cvd_fe_mul_n(int nch, uint32_t n, const uint32_t *in, uint32_t *out) {
    switch (nch) {
    case 2: return run(k_muln<2>, n, n, in, 40, out, 20);
    case 3: return run(k_muln<3>, n, n, in, 60, out, 30);
    case 4: return run(k_muln<4>, n, n, in, 80, out, 40);
    }
    return -1;
}
int cvd_fe_sq(int form, uint32_t n, const uint32_t *in, uint32_t *out) {
    switch (form) {
    case 0: return run(k_sq<0>, n, n, in, 11, out, 10);
    case 1: return run(k_sq<1>, n, n, in, 11, out, 10);
    case 2: return run(k_sq<2>, n, n, in, 11, out, 10);
    case 3: return run(k_sq<3>, n, n, in, 11, out, 10);
    }
    return -1;
}
// nch 2: fe_sq_n<2, 0>; nch 4: fe_sq_n<4, 0x4> (chain 2 doubled)
int cvd_fe_sq_n(int nch, uint32_t n, const uint32_t *in, uint32_t *out) {
    switch (nch) {
    case 2: return run(k_sqn<2, 0>, n, n, in, 20, out, 20);
    case 4: return run(k_sqn<4, 0x4>, n, n, in, 40, out, 40);
    }
    return -1;
}
int cvd_fe_sub(int form, uint32_t n, const uint32_t *in, uint32_t *out) {
    switch (form) {
    case 0: return run(k_sub<0>, n, n, in, 20, out, 10);
    case 1: return run(k_sub<1>, n, n, in, 20, out, 10);
    case 2: return run(k_sub<2>, n, n, in, 20, out, 10);
    case 3: return run(k_sub<3>, n, n, in, 20, out, 10);
    }
    return -1;
}
int cvd_fe_un(int form, uint32_t n, const uint32_t *in, uint32_t *out) {
    switch (form) {
    case 0: return run(k_un<0>, n, n, in, 10, out, 10);
    case 1: return run(k_un<1>, n, n, in, 10, out, 10);
    case 2: return run(k_un<2>, n, n, in, 10, out, 10);
    case 3: return run(k_un<3>, n, n, in, 10, out, 10);
    case 4: return run(k_un<4>, n, n, in, 10, out, 10);
    case 5: return run(k_un<5>, n, n, in, 10, out, 10);
    case 6: return run(k_un<6>, n, n, in, 10, out, 10);
    }
    return -1;
}
int cvd_fe_words(uint32_t n, const uint32_t *in, uint32_t *out) { return run(k_words, n, n, in, 18, out, 18); }

int cvd_sc_reduce(uint32_t n, const uint32_t *in, uint32_t *out) { return run(k_sc_reduce, n, n, in, 16, out, 8); }
int cvd_sc_muladd(uint32_t n, const uint32_t *in, uint32_t *out) { return run(k_sc_muladd, n, n, in, 24, out, 8); }
int cvd_exact_step(uint32_t n, const uint32_t *in, uint32_t *out) { return run(k_exact_step, n, n, in, 16, out, 9); }
int cvd_halfsize(uint32_t n, const uint32_t *in, uint32_t *out) { return run(k_halfsize, n, n, in, 16, out, 27); }
// form 0: <true, false> (tri), 1: <false, true> (throughput), 2: <false, false>
int cvd_hs_scalars(int form, uint32_t n, const uint32_t *in, uint32_t *out) {
    switch (form) {
    case 0: return run(k_hs_scalars<true, false>, n, n, in, 16, out, CV_HS_DIGWORDS);
    case 1: return run(k_hs_scalars<false, true>, n, n, in, 16, out, CV_HS_DIGWORDS);
    case 2: return run(k_hs_scalars<false, false>, n, n, in, 16, out, CV_HS_DIGWORDS);
    }
    return -1;
}
// every record's [offset, offset + length) must lie inside the arena (checked here: the kernel reads it)
int cvd_sha(uint32_t n, const uint32_t *in, uint32_t *out, const uint8_t *arena, uint32_t arena_bytes) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t *x = in + (size_t)i * 19;
        if ((x[16] != 32 && x[16] != 64) || x[17] > arena_bytes || x[18] > arena_bytes - x[17]) return -1;
    }
    return run(k_sha, n, n, in, 19, out, 24, arena, arena_bytes);
}

#endif  // part 1
#if CVD_HAS(4)
// The decode and table entry points exist twice: cvd_*_lat0 (LAT = false, the sequential-carry field forms, part 4)
// and cvd_*_lat1 (LAT = true, the latency forms of small batches, part 5).
#if CVD_PART == 5
#define CVD_LN(name) name##_lat1
#else
#define CVD_LN(name) name##_lat0
#endif
int CVD_LN(cvd_decode)(uint32_t n, const uint32_t *in, uint32_t *out) {
    return run(k_decode<CVD_LAT>, n, n, in, 8, out, 58);
}
int CVD_LN(cvd_decode2)(uint32_t n, const uint32_t *in, uint32_t *out) {
    return run(k_decode2<CVD_LAT>, n, n, in, 16, out, 98);
}
int CVD_LN(cvd_point_one)(uint32_t n, const uint32_t *in, uint32_t *out) {
    for (uint32_t i = 0; i < n; i++)
        if (in[(size_t)i * 10 + 9] > 2) return -1;
    return run(k_point_one<CVD_LAT>, n, n, in, 10, out, 364);
}
int CVD_LN(cvd_points)(uint32_t n, const uint32_t *in, uint32_t *out) {
    return run(k_points<CVD_LAT>, n, n, in, 16, out, 724);
}
#endif  // part 4
#if CVD_HAS(2)
// The quad entry points exist twice, one set per field form: cvd_quad_*_ilp (SEQ = false, part 2) and
// cvd_quad_*_seq (SEQ = true, the form production instantiates, part 3).
#if CVD_PART == 3
#define CVD_QN(name) name##_seq
#else
#define CVD_QN(name) name##_ilp
#endif
int CVD_QN(cvd_quad_dbl)(uint32_t n, const uint32_t *in, uint32_t *out) {
    return quad_run(k_quad_dbl<CVD_SEQ>, n, in, 40, out, 40);
}
// mode as k_quad_add; table: the affine rows for modes 1 and 3 when a record's "from aux" word is set.  Digits and
// table extents are checked here against the table each record names.
int CVD_QN(cvd_quad_add)(int mode, uint32_t n, const uint32_t *in, uint32_t *out, const uint32_t *table,
                         uint32_t table_words) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t *x = in + (size_t)i * 88;
        const int d = (int)x[80], m = d < 0 ? -d : d;
        if (mode == 0 || mode == 2) {
            if (m > 8) return -1;
        } else {
            const uint32_t words = x[82] ? table_words : (uint32_t)(4 * CV_BTAB_ENTRIES * CV_BTAB_STRIDE);
            const uint32_t stride = mode == 1 ? x[83] : (uint32_t)CV_BTAB_STRIDE;
            if (stride < 30 || (stride & 1) || (x[81] & 1)) return -1;
            if ((uint64_t)x[81] + (uint64_t)stride * (uint32_t)m + 30 > words) return -1;
        }
    }
    const size_t tb = (size_t)table_words * 4;
    switch (mode) {
    case 0: return quad_run(k_quad_add<CVD_SEQ, 0>, n, in, 88, out, 40, nullptr, 0, true);
    case 1: return quad_run(k_quad_add<CVD_SEQ, 1>, n, in, 88, out, 40, table, tb);
    case 2: return quad_run(k_quad_add<CVD_SEQ, 2>, n, in, 88, out, 40, nullptr, 0, true);
    case 3: return quad_run(k_quad_add<CVD_SEQ, 3>, n, in, 88, out, 40, table, tb);
    }
    return -1;
}
int CVD_QN(cvd_quad_to_cached)(uint32_t n, const uint32_t *in, uint32_t *out) {
    return quad_run(k_quad_to_cached<CVD_SEQ>, n, in, 40, out, 40);
}
// n = quads (four per 16-lane group)
int CVD_QN(cvd_tri_sum)(uint32_t n, const uint32_t *in, uint32_t *out) {
    return quad_run(k_tri_sum<CVD_SEQ>, n, in, 40, out, 40);
}
int CVD_QN(cvd_quad_chain)(uint32_t n, const uint32_t *in, uint32_t *out) {
    for (uint32_t i = 0; i < n; i++)
        for (int w = 0; w < CVD_CHAIN_WIN; w++) {
            const int d = (int)in[(size_t)i * 88 + 80 + w];
            if (d < -8 || d > 8) return -1;
        }
    return quad_run(k_quad_chain<CVD_SEQ>, n, in, 88, out, 40 * 5 * CVD_CHAIN_WIN, nullptr, 0, true);
}
#if CVD_PART == 2
int cvd_ballot(uint32_t n, const uint32_t *in, uint32_t *out) { return run(k_ballot, n, n, in, 2, out, 2); }
#endif
#endif  // part 2

}  // extern "C"
#pragma GCC visibility pop
