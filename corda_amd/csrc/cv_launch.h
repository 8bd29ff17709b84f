// cv_launch.h — internal ABI between the host library (cv_api.cpp and the cv_api_*.cpp feature units, through
// cv_host.h) and the kernel launchers (cv_kernels.hip).  Not part of the public C-ABI (include/cordaverify.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cv_ck.h"
#include "cv_notary.h"
#include "cv_tearoff.h"
#include "cv_keydedupe.h"
#include "cv_hotkeys.h"
#include "cv_keystore.h"
#include "cv_resolve.h"
#include "cv_uniq.h"

// Helper stream and events of one verify workspace slot, used by cvk_verify's drain overlap (a
// near-empty last round of a chunk is filled by a tail sub-chunk on s2).  Owned by cv_host.h's Slot (one per
// workspace slot, so two slots' calls never share a helper stream); cvk_verify only records and waits.
struct CvkSplit {
    hipStream_t s2 = nullptr;
    hipEvent_t start = nullptr, done2 = nullptr;
    int cus = 0;   // compute units of the device (resident waves per round = cus * 4 SIMDs * 3 waves)
};

// Prep overlap of a one-chunk verify (cv_api.cpp verify_shard_small): the caller records `ready` on the
// launch stream once the keys and signatures are enqueued for DMA, before the offsets, lengths and message
// bytes.  The point decodes and tables (which read only keys and signatures) wait for `ready` on `aux` and run
// beside the rest of the DMA and the scalars; the launch stream waits for `done` before the Straus kernel.
struct CvkPrepOverlap {
    hipStream_t aux = nullptr;
    hipEvent_t ready = nullptr, done = nullptr;
};

// The launch plan of one verify call, from the context's options (cv_set_option): which kernel form a
// batch of n signatures takes.  Read per call, so no launcher state is shared between contexts.
struct CvkPlan {
    uint32_t tri_max = 4096;    // n <= tri_max: tri-chain latency form (16 lanes per signature; 0 = never)
    uint32_t quad_max = 32768;  // n <= quad_max: quad latency form (4 lanes per signature; 0 = never)
    int split = 1;              // drain overlap of throughput chunks: 0 off, 1 auto (last round <= 12 % full), 2 always
    int split_pct = 10;         // the tail sub-chunk's share of a split chunk, percent
};

extern "C" {
// Verify n signatures with the workspace (capacity ws_cap signatures, a multiple of 512), in chunks of
// ws_cap.  split == nullptr disables the drain-overlap sub-chunks (the host pipeline overlaps its own
// sub-chunks across slots instead).  ev (optional, 4 events): phase boundaries of the first chunk.
// po (optional): prep overlap, taken when the batch is one chunk and ev is null (else ignored).
hipError_t cvk_verify(const CvkPlan *plan, uint32_t n, const uint8_t *pk, const uint8_t *sig, const uint8_t *arena,
                      const uint64_t *off, const uint32_t *len, uint64_t *bitmap, uint8_t *status, uint32_t *ws_tab,
                      uint8_t *ws_ok, uint32_t *ws_dig, uint32_t ws_cap, hipStream_t stream, hipEvent_t *ev,
                      const CvkSplit *split, const CvkPrepOverlap *po);
hipError_t cvk_sign(uint32_t n, const uint8_t *seed, const uint8_t *arena, const uint64_t *off, const uint32_t *len,
                    uint8_t *pk, uint8_t *sig, hipStream_t stream);
// Fixed-key signing: a signer's device record (a | prefix | abyte, then 32 bytes that carry the seed into
// cvk_key_expand and come back cleared), and n signatures with it.
#define CVK_SIGN_REC_BYTES 128
hipError_t cvk_key_expand(uint32_t *key_rec, hipStream_t stream);
hipError_t cvk_sign_keyed(uint32_t n, const uint32_t *key_rec, const uint8_t *arena, const uint64_t *off,
                          const uint32_t *len, uint8_t *sig, hipStream_t stream);
hipError_t cvk_pmt_verify(uint32_t ntrees, const uint8_t *kind, const uint32_t *left, const uint32_t *right,
                          const uint8_t *leaf_hash, const uint32_t *tree_begin, const uint8_t *root, const uint8_t *check,
                          const uint32_t *check_begin, uint32_t *dig, uint8_t *flag, uint8_t *verdict, uint8_t *status,
                          hipStream_t stream);
// Partial Merkle tree build of ntx transactions (cv_pmt_build.h): count -> scan -> emit on one stream.  The leaves are
// leaf_hash (bytes) or leaf_dig (the leaf kernel's digest words), exactly one non-null; the include lists are
// include / include_begin, or keep (one byte per leaf) when keep is non-null.  ws_off[ntx + 1]: each transaction's
// first entry of the level pyramid (dig 8 words, flag, size, pos per entry).  The node arrays must hold the
// batch's bound (cv_partial_merkle_build_bound): the kernels write tree_begin[ntx] records at the most that many.
struct CvkPmtBuild {
    const uint8_t *leaf_hash;
    const uint32_t *leaf_dig;
    const uint32_t *tx_leaf_begin;
    const uint8_t *include;
    const uint32_t *include_begin;
    const uint8_t *keep;
    const uint32_t *ws_off;
    uint32_t *dig;
    uint8_t *flag;
    uint32_t *size, *pos, *count;
    uint8_t *ids, *status;
    uint32_t *tree_begin;
    uint8_t *kind;
    uint32_t *left, *right;
    uint8_t *node_hash;
};
hipError_t cvk_pmt_build(uint32_t ntx, const CvkPmtBuild *a, hipStream_t stream);
// The uniqueness set (cv_uniq.h; kernels in cv_k_uniq.hip), every step enqueued on `stream`, nothing synchronised.
//   front : clears the batch table, then init (per request) and group + resident lookup (per state) into stat
//   round : owner = none, claim, decide stat_in -> stat_out; the requests still undecided are added to
//           dstat[CVU_D_ROUND0 + round] (zero before)
//   finish: owner = none, own, the one-wave serial tail when `tail` is set, report + insert
//   load  : phase 0 clears the batch table, groups the keys and looks them up (dstat[CVU_D_BAD] if one repeats or
//           is resident); phase 1 inserts them
//   rehash: one lane per slot of `from` re-inserts into `to` (occ of `to` zero before)
//   snapshot: count, scan and emit over the window of S; sums: CVD_LEVELS arrays of block totals (cv_kernels.hip)
hipError_t cvk_uniq_front(const CvUniqTable *T, const CvUniqBatch *B, uint32_t *stat, hipStream_t stream);
hipError_t cvk_uniq_round(const CvUniqBatch *B, const uint32_t *stat_in, uint32_t *stat_out, uint32_t round,
                          hipStream_t stream);
hipError_t cvk_uniq_finish(const CvUniqTable *T, const CvUniqBatch *B, uint32_t *stat, int tail, hipStream_t stream);
hipError_t cvk_uniq_load(const CvUniqTable *T, const CvUniqBatch *B, int phase, hipStream_t stream);
hipError_t cvk_uniq_lookup(const CvUniqTable *T, uint32_t n, const uint32_t *key, uint8_t *found, uint32_t *cons_id,
                           uint32_t *cons_index, uint32_t *cons_caller, uint32_t *dstat, hipStream_t stream);
hipError_t cvk_uniq_rehash(const CvUniqTable *from, const CvUniqTable *to, uint32_t *dstat, hipStream_t stream);
hipError_t cvk_uniq_snapshot(const CvUniqTable *T, const CvUniqSnap *S, uint32_t *const *sums, hipStream_t stream);
// Missing signers of a->ntx transactions (cv_ck.h; kernels in cv_k_ck.hip), enqueued on `stream`, nothing synchronised:
// the list's counter cleared, the narrow kernel, then (unless wide_min is UINT32_MAX) the wide kernel over the list.
// a->wide_min == 0 takes the default; count, list and flag point into the caller's workspace (cvck_ws_bytes).
hipError_t cvk_ck(const CvCk *a, hipStream_t stream);
// The notary's fused commit step (cv_notary.h; kernels in cv_k_notary.hip), every step enqueued on `stream`, nothing
// synchronised.  gate: one lane per transaction -> pre, enable, first_bad.  gather: one lane per state -> key (between
// the leaf kernel and the tree kernel: cvk_merkle with ntx == 0, then with nleaves == 0).  final: ONE workgroup ->
// outcome, the ascending list of accepted transactions with their signing records, its length in *count.  scatter:
// compact signature j -> out[list[j]] (64 bytes each; out zeroed by the caller).
hipError_t cvk_notary_gate(const CvNotary *N, hipStream_t stream);
hipError_t cvk_notary_gather(const CvNotary *N, hipStream_t stream);
hipError_t cvk_notary_final(const CvNotary *N, uint32_t *count, hipStream_t stream);
hipError_t cvk_notary_scatter(uint32_t count, const uint32_t *list, const uint8_t *sig, uint8_t *out, hipStream_t stream);
// The tear-off verifier and the oracle's signing step (cv_tearoff.h; kernels in cv_k_tearoff.hip), every step enqueued
// on `stream`, nothing synchronised.  check: one lane per filtered leaf -> the check bytes (after the leaf kernel:
// cvk_merkle with ntx == 0; nleaves == 0 launches nothing).  gate: one lane per tear-off -> outcome, first_bad and,
// where asked for, fv_verdict / fv_status (after cvk_pmt_verify).  compact: ONE workgroup -> the ascending list of
// accepted tear-offs with their signing records, its length in *count (then cvk_sign_keyed and cvk_notary_scatter).
hipError_t cvk_tearoff_check(const CvTearoff *T, hipStream_t stream);
hipError_t cvk_tearoff_gate(const CvTearoff *T, hipStream_t stream);
hipError_t cvk_tearoff_compact(const CvTearoff *T, uint32_t *count, hipStream_t stream);
// The graph steps of cv_resolve_batch (cv_resolve.h; kernels in cv_k_resolve.hip), enqueued on `stream`, nothing
// synchronised.  join: one lane per transaction inserts its claimed id into R->tab (all CVR_NONE before; R->dstat at
// its start values), then one lane per input probes it -> input_dep, input_status (ninputs == 0 launches the insert
// alone: the duplicate check is its work).  gate: one lane per transaction, after the Merkle, verify and
// missing-signers stages -> outcome, first_bad, bad_input and the counters.  Counts are at most 2^30.
hipError_t cvk_resolve_join(const CvResolve *R, hipStream_t stream);
hipError_t cvk_resolve_gate(const CvResolve *R, hipStream_t stream);
// The device key dedupe (cv_keydedupe.h; kernels in cv_k_dedupe.hip), every step enqueued on `stream`, nothing
// synchronised: D->pk[n][32] -> D->keys (the distinct keys, first-seen order; rows from the count on are not written),
// D->key_index[n], *D->nkeys (CVD_NONE after a probe error).  D->stat lies directly behind D->tab (cvd_layout) and
// sums[CVD_LEVELS] are the levels' block sums; the workspace needs no preparation.  1 <= n <= 0xfffffffe.
hipError_t cvk_dedupe(const CvDedupe *D, uint32_t *const *sums, hipStream_t stream);
// The hot-key route (cv_hotkeys.h; kernels in cv_k_hotkeys.hip), every step enqueued on `stream`, nothing synchronised.
//   front : behind cvk_dedupe over the same keys — the counters zeroed, tally, classify, the candidates' compaction, the
//           classes and hot key rows, the records' flags and their compaction -> H->head | H->hot_keys, what the host
//           reads back; sums: the dedupe's block sums (used one compaction after another).  H->hot_min >= 1.
//   gather: the stable partition of the records into H->g_* and H->perm (reads H->off / H->len: behind whatever
//           writes them)
//   merge : behind the two sub-batch verifies -> bitmap (ceil(n / 64) words, zero tail bits), status (optional)
hipError_t cvk_hotkeys_front(const CvHot *H, uint32_t *const *sums, hipStream_t stream);
hipError_t cvk_hotkeys_gather(const CvHot *H, hipStream_t stream);
hipError_t cvk_hotkeys_merge(const CvHot *H, uint64_t *bitmap, uint8_t *status, hipStream_t stream);
// The device key store (cv_keystore.h; kernels in cv_k_keystore.hip), every step enqueued on `stream`, nothing
// synchronised.  dstat: CKS_D_WORDS counters, zeroed by the caller.
//   add    : n seeds -> the staged records rec (n * CKS_REC_WORDS words) and D->pk (n * 8 words, the call's pk_out);
//            the seeds are cleared behind the expansion; then the call-local grouping over D (its table and stat
//            lie together as cvd_layout places them: one memset of 0xff), classify -> status[n], put.  The caller
//            clears rec behind it.
//   lookup : per key its slot (optional) and flag (optional: `present` for a resident key, else 1 - present)
//   rehash : one lane per slot of `from` re-inserts into `to` (occ of `to` zero before)
//   tx_gate: one lane per transaction -> X->slot / off / len per key, tx_status, first_bad
//   sign   : n signatures, record i with the key in slot[i]; CKS_NONE gives 64 zero bytes
hipError_t cvk_ks_add(const CvKeyTable *T, const CvDedupe *D, uint8_t *seed, uint32_t *rec, uint8_t *status,
                      uint32_t *dstat, hipStream_t stream);
hipError_t cvk_ks_lookup(const CvKeyTable *T, uint32_t n, const uint32_t *pk, uint32_t *slot, uint8_t *flag,
                         uint8_t present, uint32_t *dstat, hipStream_t stream);
hipError_t cvk_ks_rehash(const CvKeyTable *from, const CvKeyTable *to, uint32_t *dstat, hipStream_t stream);
hipError_t cvk_ks_tx_gate(const CvKeyTable *T, const CvKeyTx *X, hipStream_t stream);
hipError_t cvk_ks_sign(const CvKeyTable *T, uint32_t n, const uint32_t *slot, const uint8_t *arena, const uint64_t *off,
                       const uint32_t *len, uint8_t *sig, hipStream_t stream);
// Merkle ids of ntx transactions whose leaves are nleaves records starting at leaf index leaf_base:
// leaf_off / leaf_len index the records (leaf i of the call = record i), tx_begin[0..ntx] holds absolute
// leaf indices (tx_begin[0] >= leaf_base), leaf_digest is nleaves * 32 bytes of workspace.
hipError_t cvk_merkle(uint32_t ntx, uint32_t nleaves, uint32_t leaf_base, const uint8_t *arena, const uint64_t *leaf_off,
                      const uint32_t *leaf_len, const uint32_t *tx_begin, uint32_t *leaf_digest, uint8_t *ids,
                      uint8_t *status, hipStream_t stream);
// cv_verify_transactions: message references (off = 32 x the signature's transaction within the shard, len = 32)
// of shard-local signatures [c0, c0 + m); per-transaction verdicts from the shard's Merkle statuses and
// verdict bitmap.  tsb: the shard's nt + 1 absolute signature boundaries, tsb[0] = s0.
hipError_t cvk_tx_sig_refs(uint32_t m, uint32_t c0, uint32_t nt, uint32_t s0, const uint32_t *tsb, uint64_t *off,
                           uint32_t *len, hipStream_t stream);
hipError_t cvk_tx_verdicts(uint32_t nt, uint32_t s0, const uint32_t *tsb, const uint8_t *mstatus, const uint64_t *bitmap,
                           uint8_t *tx_ok, hipStream_t stream);
hipError_t cvk_calibrate(uint32_t iters, int which, uint32_t blocks, void *scratch, hipStream_t stream);
hipError_t cvk_mad_clock(uint32_t iters, uint32_t blocks, uint64_t *out, hipStream_t stream);
// Does a batch of n take the tri-chain form under this plan, in one chunk of a workspace of ws_cap?
int cvk_tri_zc_ok(const CvkPlan *plan, uint32_t n, uint32_t ws_cap);
hipError_t cvk_verify_tri_zc(const CvkPlan *plan, uint32_t n, const uint8_t *pk, const uint8_t *sig,
                             const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint8_t *nib,
                             uint8_t *status, uint32_t *ws_tab, uint8_t *ws_ok, uint32_t *ws_dig, uint32_t ws_cap,
                             hipStream_t stream, const void *copy_src, void *copy_dst, size_t copy_bytes);
hipError_t cvk_prepare(hipStream_t stream);
hipError_t cvk_keyprep(uint32_t nk, const uint8_t *keys, const uint32_t *slots, uint32_t *scratch, uint32_t *ktab_pool,
                       uint8_t *kok_pool, hipStream_t stream);
hipError_t cvk_verify_keyed(const CvkPlan *plan, uint32_t n, const uint8_t *keys, const uint32_t *key_index,
                            const uint32_t *slot_of_key, const uint32_t *ktab_pool, const uint8_t *kok_pool,
                            const uint8_t *sig, const uint8_t *arena, const uint64_t *off, const uint32_t *len,
                            uint64_t *bitmap, uint8_t *status, uint32_t *ws_hs, uint32_t *ws_R, uint8_t *ws_ok,
                            uint32_t ws_cap, hipStream_t stream, hipEvent_t *ev);
}
