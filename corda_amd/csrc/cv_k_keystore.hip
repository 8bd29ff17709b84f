// cv_k_keystore.hip — the device key store (cv_keystore.h): the expansion of a batch of seeds, the store's classify,
// put, lookup and rehash steps (a lane per record or slot), the gate of the builder's signing step (a lane per
// transaction) and many-key signing, one RFC 8032 signature per lane with the lane's OWN key record.  The call-local
// grouping of an add is the key dedupe's insert kernel (cv_k_dedupe.hip).  Shared helpers and every kernel
// declaration: cv_kcommon.h; launchers: cv_kernels.hip.
#include "cv_kcommon.h"

// n x EdDSAPrivateKeySpec(seed): one lane per seed, cv_key_expand as the fixed-key signer runs it once.  rec: the
// staged records (n * CKS_REC_WORDS, 16-byte aligned), pk: n * 8 words.  Lanes past n leave after the table is staged.
__global__ __launch_bounds__(CV_BLOCK, 2) void cv_ks_expand_kernel(uint32_t n, const uint8_t *__restrict__ seed,
                                                                   uint32_t *__restrict__ rec, uint32_t *__restrict__ pk) {
    __shared__ __attribute__((aligned(16))) uint32_t btab[CV_BTAB_ENTRIES * CV_BTAB_STRIDE];
    stage_btab(btab);
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t sd[8], a[8], prefix[8], abyte[8];
    load_words8(sd, seed + (size_t)i * 32);
    cv_key_expand(sd, a, prefix, abyte, btab);
    uint32_t *r = rec + CKS_REC_WORDS * (size_t)i;
    store_words(r + CKS_REC_A, a, 2);
    store_words(r + CKS_REC_PREFIX, prefix, 2);
    store_words(r + CKS_REC_ABYTE, abyte, 2);
    store_words(pk + 8 * (size_t)i, abyte, 2);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_ks_classify_kernel(CvKeyTable T, CvDedupe D, uint8_t *status,
                                                                  uint32_t *dstat) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < D.n) cks_classify(T, D, i, status, dstat);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_ks_put_kernel(CvKeyTable T, CvDedupe D, const uint32_t *rec,
                                                             const uint8_t *status, uint32_t *dstat) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < D.n) cks_put(T, D, i, rec, status, dstat);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_ks_lookup_kernel(CvKeyTable T, uint32_t n, const uint32_t *pk,
                                                                uint32_t *slot, uint8_t *flag, uint8_t present,
                                                                uint32_t *dstat) {
    const uint32_t i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i < n) cks_lookup(T, pk, i, slot, flag, present, dstat);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_ks_rehash_kernel(CvKeyTable from, CvKeyTable to, uint32_t *dstat) {
    const uint32_t s = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (s <= from.mask) cks_rehash(from, to, s, dstat);
}

__global__ __launch_bounds__(CV_BLOCK) void cv_ks_tx_gate_kernel(CvKeyTable T, CvKeyTx X) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t < X.ntx) cks_tx_gate(T, X, t);
}

// One message per lane, signed with the record of the lane's slot.  A lane without a slot (its key is absent, or its
// transaction is abandoned) writes 64 zero bytes and leaves before any read of the store.  The record's three parts
// are handed to cv_sign_keyed_one as pointers into the store, so each is loaded where it is consumed — prefix before
// the first hash, Abyte before the second, a at sc_muladd — and none of the 24 words is live across the scalar
// multiplication.  Two waves per SIMD, as cv_sign_keyed_kernel (DESIGN.md §5.16 quotes the compiler's numbers).
__global__ __launch_bounds__(CV_BLOCK, CV_SIGN_WAVES) void cv_ks_sign_kernel(
    CvKeyTable T, uint32_t n, const uint32_t *__restrict__ slot, const uint8_t *__restrict__ arena,
    const uint64_t *__restrict__ off, const uint32_t *__restrict__ len, uint8_t *__restrict__ sig_out,
    const uint32_t *__restrict__ bw16) {
    const uint32_t gid = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (gid >= n) return;
    uint32_t *out = reinterpret_cast<uint32_t *>(sig_out + (size_t)gid * 64);
    const uint32_t s = slot[gid];
    uint32_t sgw[16];
    if (s == CKS_NONE || s > T.mask) {
#pragma unroll
        for (int q = 0; q < 16; q++) sgw[q] = 0;
        store_words(out, sgw, 4);
        return;
    }
    const uint32_t *rec = T.rec + CKS_REC_WORDS * (size_t)s;
    cv_sign_keyed_one(bw16, rec + CKS_REC_A, rec + CKS_REC_PREFIX, rec + CKS_REC_ABYTE, arena + off[gid], len[gid], sgw);
    store_words(out, sgw, 4);
}
