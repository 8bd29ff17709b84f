// cv_k_sign.hip — fixed-key batch signing (cv_signer / cv_ed25519_sign_keyed): the signer's key expansion and
// one RFC 8032 signature per lane from the expanded key and the per-device CV_BW16 basepoint rows.
// Shared helpers and every kernel declaration: cv_kcommon.h; launchers: cv_kernels.hip.
#include "cv_kcommon.h"

// Key expansion, once per signer and device.  rec: CV_SIGN_REC_WORDS words — the caller puts the seed in
// words 24..31; lane 0 writes the key record a | prefix | abyte (words 0..23) and clears the seed words.
__global__ __launch_bounds__(CV_BLOCK) void cv_key_expand_kernel(uint32_t *__restrict__ rec) {
    __shared__ __attribute__((aligned(16))) uint32_t btab[CV_BTAB_ENTRIES * CV_BTAB_STRIDE];
    stage_btab(btab);
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t seed[8], a[8], prefix[8], abyte[8];
#pragma unroll
    for (int q = 0; q < 8; q++) seed[q] = rec[24 + q];
    cv_key_expand(seed, a, prefix, abyte, btab);
    store_words(rec, a, 2);
    store_words(rec + 8, prefix, 2);
    store_words(rec + 16, abyte, 2);
    uint4 *z = reinterpret_cast<uint4 *>(rec + 24);
    z[0] = z[1] = make_uint4(0, 0, 0, 0);
}

// One message per lane.  The key record is the same for every lane: its 24 words are read through a
// wave-uniform pointer (scalar loads, held in SGPRs), so a lane's live state is one point, one table entry,
// the hash state and three scalars.  Two waves per SIMD: the most at which the kernel keeps everything in
// registers (DESIGN.md §5.8 quotes the compiler's numbers).  Lanes past n leave before any memory access.
__global__ __launch_bounds__(CV_BLOCK, CV_SIGN_WAVES) void cv_sign_keyed_kernel(
    uint32_t n, const uint32_t *__restrict__ key_rec, const uint8_t *__restrict__ arena,
    const uint64_t *__restrict__ off, const uint32_t *__restrict__ len, uint8_t *__restrict__ sig_out,
    const uint32_t *__restrict__ bw16) {
    const uint32_t gid = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (gid >= n) return;
    uint32_t a[8], prefix[8], abyte[8], sgw[16];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        a[q] = key_rec[q];
        prefix[q] = key_rec[8 + q];
        abyte[q] = key_rec[16 + q];
    }
    cv_sign_keyed_one(bw16, a, prefix, abyte, arena + off[gid], len[gid], sgw);
    store_words(reinterpret_cast<uint32_t *>(sig_out + (size_t)gid * 64), sgw, 4);
}
