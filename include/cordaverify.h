/*
 * cordaverify.h — C-ABI of the MI355X batched signature-verification engine for Corda's
 * transaction-validation hot path.  Plain pointers and sizes only (no C++ / torch types), so the
 * JVM binds it directly through JNA or JNI (binding stubs: INTEGRATION.md).
 *
 * What each entry point replaces in the reference (MarioAriasC/corda @ 0.7-SNAPSHOT):
 *
 *   cv_ed25519_verify_batch   N x  PublicKey.verifyWithECDSA(content, signature)
 *                                 core/src/main/kotlin/net/corda/core/crypto/CryptoUtilities.kt:90-96
 *                             i.e. net.i2p.crypto:eddsa:0.1.0 EdDSAEngine.initVerify/update/verify
 *                             (jar pinned at core/build.gradle:80), looped sequentially by
 *                             SignedTransaction.checkSignaturesAreValid()
 *                                 core/src/main/kotlin/net/corda/core/transactions/SignedTransaction.kt:82-87
 *                             and by the notary / resolve flows (NotaryFlow.kt:97-113,
 *                             ValidatingNotaryFlow.kt:24-45, ResolveTransactionsFlow.kt:105-111).
 *                             Verdicts are bit-exact with eddsa-0.1.0, adversarial inputs included.
 *   cv_merkle_tx_ids          N x  WireTransaction.id  (= MerkleTree.getMerkleTree(leafHashes).hash)
 *                                 core/src/main/kotlin/net/corda/core/transactions/WireTransaction.kt:45-52
 *                                 core/src/main/kotlin/net/corda/core/transactions/MerkleTransaction.kt:26-38,66-99
 *                             leaf hash = SecureHash.sha256(leaf bytes)  (core/.../crypto/SecureHash.kt:33)
 *   cv_ed25519_sign_batch     N x  PrivateKey.signWithECDSA(bytes) after entropyToKeyPair/seed
 *                                 CryptoUtilities.kt:63-73,123-130 (deterministic RFC 8032; used to
 *                                 generate synthetic workloads, not on the validation path)
 *   cv_signer_open +          N x  KeyPair.signWithECDSA(bytes) with ONE long-lived key
 *   cv_ed25519_sign_keyed         CryptoUtilities.kt:63-73,80-87: the notary's reply signatures, sign(stx.id) and
 *                                 the signed conflict report (NotaryFlow.kt:97-113,133-141; SignedData.kt),
 *                                 and every node's own-key signing.  The same RFC 8032 signatures as
 *                                 cv_ed25519_sign_batch, with the key expanded once.
 *   cv_tx_verdicts            per-transaction AND of signature verdicts (the "all sigs valid" half of
 *                                 SignedTransaction.verifySignatures, SignedTransaction.kt:58-72)
 *   cv_verify_transactions    N x  SignedTransaction.verifySignatures' id + signature checks in one call
 *                                 (SignedTransaction.kt:59-71, 83-87; WireTransaction.kt:45-52)
 *   cv_partial_merkle_verify  N x  PartialMerkleTree.verify(merkleRootHash, hashesToCheck)
 *                                 core/src/main/kotlin/net/corda/core/crypto/PartialMerkleTree.kt:117-144
 *                             behind FilteredTransaction.verify (MerkleTransaction.kt:170-178; the
 *                             oracle tear-off check of NodeInterestRates.kt:189-191)
 *   cv_partial_merkle_build   N x  PartialMerkleTree.build(merkleRoot, includeHashes)
 *                                 PartialMerkleTree.kt:69-111 over MerkleTree.getMerkleTree (MerkleTransaction.kt:66-99)
 *   cv_filtered_build         N x  FilteredTransaction.buildMerkleTransaction (MerkleTransaction.kt:146-168): leaf
 *                                 hashes, full tree and pruned tree of every tear-off in one call
 *   cv_filtered_verify        N x  FilteredTransaction.verify(merkleRoot) from the filtered leaves' bytes
 *                                 MerkleTransaction.kt:112-117,173-178 with PartialMerkleTree.kt:118-144: the
 *                                 filtered hashes are made on the device
 *   cv_tearoff_sign_batch     N x  NodeInterestRates.Oracle.sign(ftx, merkleRoot)
 *                                 samples/irs-demo/src/main/kotlin/net/corda/irs/api/NodeInterestRates.kt:190-225
 *                                 (client: RatesFixFlow.kt:100-110): the tear-off verified, the oracle's refusals in
 *                                 the reference's order and the root signed with its fixed key, in one call
 *   cv_uniq_open +            N x  UniquenessProvider.commit(states, txId, callerIdentity)
 *   cv_uniq_commit_batch          core/src/main/kotlin/net/corda/core/node/services/UniquenessProvider.kt:13-35 as
 *                                 InMemoryUniquenessProvider.kt:14-36 decides it (the decision half of
 *                                 PersistentUniquenessProvider.kt:61-81), for NotaryFlow.kt:133-141: a device-resident
 *                                 set of consumed states, a batch decided exactly as sequential commits would
 *   cv_uniq_snapshot +             DistributedImmutableMap.snapshot / install
 *   cv_uniq_install               node/src/main/kotlin/net/corda/node/services/transactions/DistributedImmutableMap.kt:
 *                                 87-105, the state machine of RaftUniquenessProvider.kt:44-129: the set's entries
 *                                 read out in chunks, and a set that takes over a snapshot's contents in one step
 *   cv_missing_signers        N x  SignedTransaction.getMissingSignatures() and the verdict verifySignatures draws from it
 *                                 core/src/main/kotlin/net/corda/core/transactions/SignedTransaction.kt:58-72,89-93
 *                                 (tx.mustSign.filter { !it.isFulfilledBy(sigKeys) } minus allowedToBeMissing) over
 *                                 weighted-threshold CompositeKey trees, core/.../crypto/CompositeKey.kt:22-108
 *                                 (Leaf.isFulfilledBy :49, Node.isFulfilledBy :75-81)
 *   cv_notarise_batch         N x  NotaryFlow.Service.call with ValidatingNotaryFlow.beforeCommit's signature checks
 *                                 core/src/main/kotlin/net/corda/flows/NotaryFlow.kt:96-146, ValidatingNotaryFlow.kt:24-45,
 *                                 SignedTransaction.kt:34-38,58-93: ids, signatures, missing signers, the commit and
 *                                 the notary's signatures for a whole batch in one call, the reference's outcome and
 *                                 precedence settled in the library
 *   cv_resolve_batch          1 x  ResolveTransactionsFlow.call over the downloaded transactions
 *                                 core/src/main/kotlin/net/corda/flows/ResolveTransactionsFlow.kt:37-67,96-111,170,
 *                                 SignedTransaction.kt:34-38,58-93,134, ServiceHub.kt:46-49: ids, signatures, missing
 *                                 signers, the join of every input against the batch, the duplicate check,
 *                                 topologicalSort and the ordered walk up to its first failure in one call
 *   cv_keystore_open +        N x  KeyManagementService.freshKey() / keys.contains(pk) / toKeyPair(pk).signWithECDSA(bytes)
 *   cv_keystore_add / _sign       core/src/main/kotlin/net/corda/core/node/services/Services.kt:206-219 as
 *                                 PersistentKeyManagementService.kt:40-66 keeps it: a device-resident store of expanded
 *                                 private keys addressed by public key, every signed record naming its own key
 *   cv_sign_transactions      N x  the flows' signing loop and the builder's id (CashFlow.kt:39-47,
 *                                 TwoPartyTradeFlow.kt:227-235, TransactionBuilder.kt:93-98,132-141): ids from the
 *                                 leaves, then every named key's signature over the id, in one call
 *
 * Conventions
 *   - Return codes: CV_OK (0) or a negative CV_E* code; nothing throws, aborts or longjmps across
 *     the ABI.  cv_strerror() gives a static message.
 *   - Host-buffer calls are synchronous unless named _async; the caller owns every buffer.  A cv_ctx is
 *     thread-safe: calls from several threads run concurrently on different devices (each device has
 *     its own lock and worker thread) and queue on the same one.  A notary's batching threads share one
 *     context (the JVM shim holds one ctx per process, no mutex around it).
 *   - Record layout (structure-of-arrays): pk[n][32], sig[n][64] (R || S), message i is
 *     msg_arena[msg_off[i] .. msg_off[i] + msg_len[i]).
 *   - verdict_bitmap: ceil(n/64) uint64 words, bit (i % 64) of word (i / 64) = signature i valid.
 *   - status (optional, may be NULL): one byte per signature, CV_SIG_OK or CV_SIG_BAD_KEY (the key
 *     bytes are not a valid point: the reference throws IllegalArgumentException when building the
 *     EdDSAPublicKey).  Length errors (sig != 64 B -> SignatureException, key != 32 B) cannot be
 *     expressed in these fixed-width records; the host shim rejects them before the call.
 *   - Outputs, both APIs (tests/test_gpu_output_contract.py, tests/test_gpu_host_output_contract.py):
 *       prior contents  Outputs may hold anything on entry: a successful call writes every byte of every output
 *                       it is given (of the node arrays: the *nnodes entries used) and nothing before or behind
 *                       it; it never ORs into, or relies on, what was there.  Inputs are only read.
 *       tail bits       The bits of the last bitmap word at and above n are written as zero.
 *       empty tx        The id of a transaction without leaves (CV_TX_EMPTY) is 32 zero bytes.
 *       nothing to do   A count of 0 returns CV_OK and writes no output byte; neither does the CV_E_ARGS return of
 *                       a bounded call without a ticket whose records reach past the arena, nor CV_E_OOM of the
 *                       uniqueness set.
 *     Host arrays need the alignment of their C type and no more (the device-resident API: see its section).
 *   - Multi-GPU: cv_open(mask) with several bits set routes host-buffer batches over the devices: a batch
 *     up to CV_OPT_SHARD_MIN records goes whole to the least loaded device; a throughput batch (from
 *     CV_OPT_SPREAD_MIN records) is cut into contiguous ranges (multiples of 64) over all of them; a batch
 *     between the two is cut over the devices idle at submission (at most ceil(n / CV_OPT_SHARD_MIN) of
 *     them, at least the least loaded one).  No collective: each shard's results land in the caller's
 *     arrays.
 */
#ifndef CORDAVERIFY_H
#define CORDAVERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CV_OK 0
#define CV_E_NO_DEVICE (-1)   /* no HIP device matches the mask */
#define CV_E_HIP (-2)         /* a HIP runtime call failed */
#define CV_E_ARGS (-3)        /* null pointer / bad size */
#define CV_E_OOM (-4)         /* device allocation failed */
#define CV_E_TOO_LARGE (-5)   /* more than 2^32-1 records in one shard */

#define CV_SIG_OK 0
#define CV_SIG_BAD_KEY 1
#define CV_TX_OK 0
#define CV_TX_EMPTY 1         /* no leaves: MerkleTreeException("Cannot calculate Merkle root on empty hash list.") */

typedef struct cv_ctx cv_ctx;

/* Open a context on the devices in device_mask (bit d = HIP device ordinal d; 0 = all devices).
 * The first open on a device also builds that device's basepoint rows (16.8 MB, kept for the
 * process lifetime, shared by every context), so it takes a few milliseconds longer. */
int cv_open(uint32_t device_mask, cv_ctx **out);
/* As cv_open; slots_per_device (1..16) > 1 makes each GPU of the mask appear that many times in THIS context
 * as independent device slots (own lock, worker thread, streams, workspaces, key pool), so the multi-device
 * routing below runs on a one-GPU machine (tests).  slots_per_device = 1 is cv_open. */
int cv_open_ex(uint32_t device_mask, int slots_per_device, cv_ctx **out);
void cv_close(cv_ctx *ctx);
const char *cv_strerror(int code);
const char *cv_version(void);
/* Number of devices in the context. */
int cv_device_count(const cv_ctx *ctx);

/* ---------------------------------------------------------------- host-buffer API (JVM drop-in) */

int cv_ed25519_verify_batch(cv_ctx *ctx, size_t n, const uint8_t *pk, const uint8_t *sig,
                            const uint8_t *msg_arena, const uint64_t *msg_off, const uint32_t *msg_len,
                            uint64_t *verdict_bitmap, uint8_t *status);

/* Asynchronous form of cv_ed25519_verify_batch (same records, same verdicts and status, the same
 * automatic keyed path for batches whose keys repeat): enqueues the batch on the context's devices and
 * returns a ticket; cv_wait(ticket) returns once verdict_bitmap and status hold the results.  Until then
 * the caller keeps every array of the call alive and unmodified (pinned inputs are read by DMA after this
 * call returns).  Four pipelined calls (verify or Merkle) per device may be in flight: a fifth first
 * completes the oldest (whose cv_wait then returns at once).  A node's batching loop submits batch k+1
 * before waiting for batch k, so its copies and kernels fill the first one's pipeline ramp and tail.
 * cv_wait may run on another thread than the submission and does not block submissions.  It returns the
 * call's own status — also when a later call already completed it (a HIP failure while finishing a call is
 * reported to that call's waiter, never to the later caller).  Tickets are waited at most once (again:
 * CV_E_ARGS); a completed ticket keeps its status for cv_wait until 4,096 later tickets have completed;
 * cv_close drops results not yet waited for. */
int cv_ed25519_verify_batch_async(cv_ctx *ctx, size_t n, const uint8_t *pk, const uint8_t *sig,
                                  const uint8_t *msg_arena, const uint64_t *msg_off, const uint32_t *msg_len,
                                  uint64_t *verdict_bitmap, uint8_t *status, uint64_t *ticket);
int cv_wait(cv_ctx *ctx, uint64_t ticket);

/* cv_ed25519_verify_batch (ticket NULL) or its _async form (ticket non-NULL) with the arena's size: a call whose
 * records reach past msg_arena[arena_bytes) returns CV_E_ARGS before the engine reads past it.  The check rides on
 * the staging scan every call makes anyway (the byte range its records reach, per shard and sub-chunk), so a
 * binding gets bounds safety without scanning the offsets itself (cv_msg_extent, an extra pass over 12 B per
 * record).  With a ticket, records past the bound in a later shard may be found after earlier shards were
 * enqueued: the call then waits for those before it returns CV_E_ARGS. */
int cv_ed25519_verify_batch_ex(cv_ctx *ctx, size_t n, const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_arena,
                               uint64_t arena_bytes, const uint64_t *msg_off, const uint32_t *msg_len,
                               uint64_t *verdict_bitmap, uint8_t *status, uint64_t *ticket);

/* Pinned host memory for the host-buffer API's inputs (hipHostMalloc).  When all five input arrays of
 * cv_ed25519_verify_batch lie in pinned memory (from here, or any page-locked / registered host memory),
 * the engine DMAs each sub-chunk's records straight out of them and skips its packing copy into its own
 * staging: a JVM shim that builds its batches in buffers from cv_host_alloc (JNA Pointer ->
 * ByteBuffer) feeds the GPU at PCIe rate.  The memory stays valid until cv_host_free; ctx only selects
 * the allocator (any open context). */
int cv_host_alloc(cv_ctx *ctx, size_t bytes, void **out);
void cv_host_free(cv_ctx *ctx, void *p);

/* Keyed batch: the distinct keys once, keys[nkeys][32], and per signature
 * key_index[n] into them.  Replaces the same N x PublicKey.verifyWithECDSA as
 * cv_ed25519_verify_batch — identical verdicts and status — for batches whose keys repeat (a notary
 * batch, a ResolveTransactionsFlow chain, a party's transactions): the engine keeps per-key tables
 * (decoded A and comb multiples k * 2^(64j) * (-A), k = 0..128, 66 KB per key, affine) resident on each
 * device, keyed by the 32 key bytes, so a key is decoded once and each verify needs 56 doublings
 * instead of 252.
 * cv_ed25519_verify_batch(_async) takes this path by itself (host-side dedupe, any batch size above
 * CV_OPT_TRI_MAX) for batches with at least eight signatures per distinct key. */
int cv_ed25519_verify_batch_keyed(cv_ctx *ctx, size_t n, size_t nkeys, const uint8_t *keys, const uint32_t *key_index,
                                  const uint8_t *sig, const uint8_t *msg_arena, const uint64_t *msg_off,
                                  const uint32_t *msg_len, uint64_t *verdict_bitmap, uint8_t *status);

/* Per-device key-table pool capacity in keys (default 16384 = 1.1 GB of HBM per device: 66 KB of
 * comb tables per key); takes effect at the next keyed call.  A pool that fills up is emptied before
 * new keys go in; a call with more distinct keys than the capacity grows the pool to fit them. */
int cv_key_cache_reserve(cv_ctx *ctx, size_t max_keys);

/* out4 = {resident keys, capacity, lookups that hit, lookups that missed} for `device`.  One lookup per key
 * row of a call: every row of the device-resident call's d_keys, and of the host-buffer calls the rows that some
 * signature of the shard references (the others are never read).  A key already resident hits; of the rows of one
 * call that hold the same new key, the first misses (its tables are computed once) and the others hit. */
int cv_key_cache_stats(cv_ctx *ctx, int device, uint64_t *out4);

int cv_merkle_tx_ids(cv_ctx *ctx, size_t ntx, const uint8_t *leaf_arena, const uint64_t *leaf_off,
                     const uint32_t *leaf_len, const uint32_t *tx_leaf_begin /* ntx+1 */, uint8_t *ids /* ntx*32 */);

/* as cv_merkle_tx_ids, with per-transaction status (CV_TX_OK / CV_TX_EMPTY).  Transactions are cut into
 * contiguous ranges over the context's devices (routed as the verify batches), each range's leaves copied
 * from its own byte window of leaf_arena (offsets need not be sorted; scattered leaves are gathered) and
 * pipelined through the devices' copy streams in sub-chunks of about CV_OPT_MERKLE_CHUNK leaves; leaf
 * arrays in pinned memory (cv_host_alloc) are DMAed in place. */
int cv_merkle_tx_ids_ex(cv_ctx *ctx, size_t ntx, const uint8_t *leaf_arena, const uint64_t *leaf_off,
                        const uint32_t *leaf_len, const uint32_t *tx_leaf_begin, uint8_t *ids, uint8_t *tx_status);

/* Asynchronous form of cv_merkle_tx_ids_ex (ticket and cv_wait as cv_ed25519_verify_batch_async): a C3 node
 * step submits the Merkle ids of batch k+1 while the verify of batch k runs, so their copies overlap. */
int cv_merkle_tx_ids_async(cv_ctx *ctx, size_t ntx, const uint8_t *leaf_arena, const uint64_t *leaf_off,
                           const uint32_t *leaf_len, const uint32_t *tx_leaf_begin, uint8_t *ids, uint8_t *tx_status,
                           uint64_t *ticket);

/* cv_merkle_tx_ids_ex (ticket NULL) or cv_merkle_tx_ids_async (ticket non-NULL) with the leaf arena's size: a call
 * whose leaves reach past leaf_arena[leaf_arena_bytes) (or whose off + len wraps) returns CV_E_ARGS before the
 * engine reads past it — the check rides on the staging scan of each sub-chunk's leaves, so a binding needs no
 * scan of its own (6M leaves: ~10 ms of host time per call).  With a ticket, leaves past the bound in a later
 * sub-chunk may be found after earlier ones were enqueued: the call then waits for those before returning. */
int cv_merkle_tx_ids_bounded(cv_ctx *ctx, size_t ntx, const uint8_t *leaf_arena, uint64_t leaf_arena_bytes,
                             const uint64_t *leaf_off, const uint32_t *leaf_len, const uint32_t *tx_leaf_begin,
                             uint8_t *ids, uint8_t *tx_status, uint64_t *ticket);

/* Partial Merkle trees (FilteredTransaction / PartialMerkleTree.verify), one verdict per tree.
 * The shim flattens each PartialTree object in post-order and concatenates the trees: node k has
 * kind[k] (CV_PMT_LEAF 0 = PartialTree.Leaf, CV_PMT_INCLUDED 1 = IncludedLeaf, CV_PMT_NODE 2 = Node),
 * for a Node left[k] / right[k] = absolute indices of its children (smaller than k, inside the same
 * tree), for a leaf leaf_hash[k][32] = its SecureHash bytes; tree t is nodes
 * [tree_begin[t], tree_begin[t+1]) with its root last.  root[t][32] = merkleRootHash, the
 * hashesToCheck of tree t are check[check_begin[t] .. check_begin[t+1]).
 * verdict[t] = 1 iff hashConcat recomputation gives root[t] AND the IncludedLeaf hashes equal the
 * check hashes as a multiset (the reference's groupBy compare).  status[t] (optional) = CV_PMT_OK,
 * or CV_PMT_MALFORMED when the nodes are not a tree encoding (verdict 0; the shim throws
 * IllegalArgumentException).  FilteredTransaction.verify's empty-check MerkleTreeException stays in
 * the shim. */
#define CV_PMT_OK 0
#define CV_PMT_MALFORMED 2
int cv_partial_merkle_verify(cv_ctx *ctx, size_t ntrees, size_t nnodes, const uint8_t *kind, const uint32_t *left,
                             const uint32_t *right, const uint8_t *leaf_hash /* nnodes*32 */,
                             const uint32_t *tree_begin /* ntrees+1 */, const uint8_t *root /* ntrees*32 */,
                             size_t ncheck, const uint8_t *check /* ncheck*32 */,
                             const uint32_t *check_begin /* ntrees+1 */, uint8_t *verdict /* ntrees */,
                             uint8_t *status /* ntrees, optional */);

/* Partial Merkle tree BUILD (tear-offs, the prover side): for every transaction the full tree of
 * MerkleTree.getMerkleTree (MerkleTransaction.kt:66-99: a level's odd last node gets a DuplicatedLeaf with its own
 * hash as right sibling) pruned by PartialMerkleTree.build (PartialMerkleTree.kt:69-111), written in the flat
 * encoding cv_partial_merkle_verify reads, so a build's outputs are a verify's inputs as they stand.
 *   - A leaf becomes an IncludedLeaf iff its hash occurs in the include list (by hash, not position; a
 *     DuplicatedLeaf never); a node above an IncludedLeaf becomes a Node (32 zero bytes in node_hash), every other
 *     subtree is cut to a Leaf with its hash; for leaves left = right = 0.
 *   - status[t]: CV_PMT_OK; CV_PMT_EMPTY for no leaves; CV_PMT_NOT_IN_TREE iff the number of IncludedLeaves differs
 *     from the include list's length (an absent hash, a hash listed twice for one leaf, a listed hash that several
 *     leaves carry) — the reference's MerkleTreeException messages.  An empty include list is legal: one Leaf(root).
 *   - tree_begin[ntx+1]: transaction t's nodes are [tree_begin[t], tree_begin[t+1]), root last; a transaction whose
 *     status is not CV_PMT_OK has none.  *nnodes = tree_begin[ntx].
 *   - ids[t][32] (optional): the Merkle root (WireTransaction.id) of every transaction with a leaf, zero bytes for
 *     CV_PMT_EMPTY.
 *   - nodes_cap: the capacity of kind / left / right / node_hash in nodes.  If the batch needs more, the call
 *     writes tree_begin, status, ids and *nnodes, leaves the node arrays alone and returns CV_E_ARGS; a caller
 *     that allocates cv_partial_merkle_build_bound nodes never sees this.
 * Synchronous, on one device (the least loaded).  Ranges as cv_partial_merkle_verify: begin[0] == 0, monotone
 * (CV_E_ARGS otherwise); more than 0xfffffffe transactions, leaves, include hashes or nodes of the bound:
 * CV_E_TOO_LARGE.  ntx == 0 returns CV_OK and touches nothing. */
#define CV_PMT_EMPTY 1          /* no leaves: MerkleTreeException("Cannot calculate Merkle root on empty hash list.") */
#define CV_PMT_NOT_IN_TREE 3    /* MerkleTreeException("Some of the provided hashes are not in the tree.") */

/* host only: the sum over the transactions of the most nodes a build can emit (all leaves included) — for L leaves
 * the entries of all levels plus one per level with an odd count above 1 (13 for L = 5, 141 for L = 65) */
uint64_t cv_partial_merkle_build_bound(size_t ntx, const uint32_t *tx_leaf_begin /* ntx+1 */);

/* N x PartialMerkleTree.build(MerkleTree.getMerkleTree(leafHashes), includeHashes)  (PartialMerkleTree.kt:69-111) */
int cv_partial_merkle_build(cv_ctx *ctx, size_t ntx, const uint8_t *leaf_hash /* nleaves*32 */,
                            const uint32_t *tx_leaf_begin /* ntx+1 */, const uint8_t *include /* ninclude*32 */,
                            const uint32_t *include_begin /* ntx+1 */, size_t nodes_cap, uint8_t *kind, uint32_t *left,
                            uint32_t *right, uint8_t *node_hash /* nodes_cap*32 */, uint32_t *tree_begin /* ntx+1 */,
                            uint8_t *ids /* ntx*32, optional */, uint8_t *status /* ntx */, size_t *nnodes);

/* N x FilteredTransaction.buildMerkleTransaction (MerkleTransaction.kt:146-168; caller RatesFixFlow.kt:100-110): the
 * leaf blobs as cv_merkle_tx_ids_bounded takes them (hashed by the same leaf kernel; leaves past
 * leaf_arena[leaf_arena_bytes) or wrapping give CV_E_ARGS before any read), keep[nleaves] = the FilterFuns' verdict
 * per leaf (non-zero: kept).  The include list of a transaction is the hashes of its kept leaves, so a leaf is
 * included iff its hash equals a kept leaf's, and a kept leaf whose bytes another leaf repeats gives
 * CV_PMT_NOT_IN_TREE as in the reference.  Outputs as cv_partial_merkle_build. */
int cv_filtered_build(cv_ctx *ctx, size_t ntx, const uint8_t *leaf_arena, uint64_t leaf_arena_bytes,
                      const uint64_t *leaf_off, const uint32_t *leaf_len, const uint32_t *tx_leaf_begin /* ntx+1 */,
                      const uint8_t *keep /* nleaves */, size_t nodes_cap, uint8_t *kind, uint32_t *left,
                      uint32_t *right, uint8_t *node_hash /* nodes_cap*32 */, uint32_t *tree_begin /* ntx+1 */,
                      uint8_t *ids /* ntx*32, optional */, uint8_t *status /* ntx */, size_t *nnodes);

int cv_ed25519_sign_batch(cv_ctx *ctx, size_t n, const uint8_t *seed /* n*32 */, const uint8_t *msg_arena,
                          const uint64_t *msg_off, const uint32_t *msg_len, uint8_t *pk_out /* n*32 */,
                          uint8_t *sig_out /* n*64 */);

/* A signer: one Ed25519 private key (EdDSAPrivateKeySpec(seed), the KeyPair of entropyToKeyPair / generateKeyPair,
 * CryptoUtilities.kt:117-130) expanded once on every device of the context — the clamped scalar a, the hash prefix
 * and the encoded public key A = [a]B: a 128-byte device record per device (96 bytes of key record, and 32 bytes
 * that carry the seed to the expansion kernel, which clears them).  It is what a notary holds for its
 * replies (NotaryFlow.kt:97-113: sign(stx.id); :133-141: the SignedData conflict report, SignedData.kt) and a node
 * for its own signatures (PrivateKey.signWithECDSA, CryptoUtilities.kt:63-73).
 * cv_signer_open returns the usual codes; the seed is copied to the devices through pinned memory that is wiped
 * before the call returns, and the library keeps no host copy of the seed, a or the prefix.  The wiping covers
 * what the library allocates: the expansion kernel also uses 48 bytes per lane of the device's scratch memory
 * (as cv_ed25519_sign_batch's kernel uses 112), where words derived from the seed may remain until the device
 * reuses it; the signing kernel itself uses no scratch.  A signer is immutable
 * after open: any number of threads may sign with it at once, under the context's rules above.  cv_signer_close
 * waits for the devices, overwrites the device records and frees them (NULL: no-op); a signer is closed before
 * its context. */
typedef struct cv_signer cv_signer;
int cv_signer_open(cv_ctx *ctx, const uint8_t seed[32], cv_signer **out);
/* The signer's public key, KeyPair.public's 32 encoded bytes (EdDSAPublicKey.abyte; CryptoUtilities.kt:71-73, 80). */
int cv_signer_public_key(const cv_signer *s, uint8_t pk[32]);
void cv_signer_close(cv_signer *s);

/* N x KeyPair.signWithECDSA(bytesToSign) with the signer's key (CryptoUtilities.kt:63-73, 80; the notary's
 * NotaryFlow.kt:97-113 replies in one call): RFC 8032 deterministic signatures, bit for bit those of
 * cv_ed25519_sign_batch with the seed repeated n times, sig_out[i] = R || S over message i.  The batch is routed
 * over the context's devices like cv_ed25519_sign_batch (shards in multiples of 64).  n == 0 returns CV_OK and
 * touches nothing; a record whose msg_off + msg_len exceeds msg_arena_bytes, or wraps, returns CV_E_ARGS before
 * any copy or launch (msg_arena_bytes = UINT64_MAX: unchecked). */
int cv_ed25519_sign_keyed(cv_ctx *ctx, const cv_signer *s, size_t n, const uint8_t *msg_arena,
                          uint64_t msg_arena_bytes, const uint64_t *msg_off, const uint32_t *msg_len,
                          uint8_t *sig_out /* n*64 */);

/* A uniqueness set: the notary's map of consumed states (InMemoryUniquenessProvider.committedStates,
 * node/src/main/kotlin/net/corda/node/services/transactions/InMemoryUniquenessProvider.kt:14-36; the table of
 * PersistentUniquenessProvider.kt:19-81), resident on ONE device of the context: `device` is an index into the
 * context's devices (0 for a context of one).  It maps a 32-byte state key, all 32 bytes the identity, to the
 * consuming record UniquenessProvider.ConsumingTx(id[32], inputIndex u32, requestingParty) (UniquenessProvider.kt:31);
 * the party is a u32 handle, the binding keeps the Party table.  The binding chooses the key; the documented
 * choice is SecureHash.sha256 of the serialised StateRef (Structures.kt:337), the input's Merkle leaf hash.
 *   - Open addressing over a power-of-two slot count of at least 2 x capacity (16 at the least), about 76 bytes a
 *     slot.  Slots are chosen by a hash of the whole key mixed with a per-set random seed, never by key bits: keys
 *     are SHA-256 outputs a submitter can grind.  No single entry is deleted; cv_uniq_clear and cv_uniq_install
 *     replace the whole contents.
 *   - A call that would take the set past its capacity (resident + the call's states, repeats included) returns
 *     CV_E_OOM before any change to the set and before any output is written; cv_uniq_reserve makes room (a rehash
 *     on the device into a larger table; it never shrinks).
 *   - Calls on one set serialise on a mutex in the set (the reference's ThreadBox); all are synchronous.  The set
 *     has a stream and a workspace of its own, so it runs beside the context's other calls.  It is not durable: a
 *     restarted notary warms it with cv_uniq_load from its commit log, or with cv_uniq_install from a snapshot
 *     (cv_uniq_snapshot) that it or another replica wrote.
 *   - More than 0xfffffffe requests, states or keys: CV_E_TOO_LARGE; so is a capacity, or one call, of more than
 *     2^30 states.  A count of 0 returns CV_OK and touches nothing.  cv_uniq_close(NULL) is a no-op; a set is
 *     closed before its context. */
typedef struct cv_uniq cv_uniq;
#define CV_UNIQ_OK 0
#define CV_UNIQ_CONFLICT 1
#define CV_UNIQ_SKIPPED 2
int cv_uniq_open(cv_ctx *ctx, int device, size_t capacity_states, cv_uniq **out);
void cv_uniq_close(cv_uniq *u);
int cv_uniq_reserve(cv_uniq *u, size_t capacity_states);

/* N x UniquenessProvider.commit(states, txId, callerIdentity) (UniquenessProvider.kt:13-35; NotaryFlow.kt:133-141
 * commitInputStates), decided EXACTLY as ntx sequential commit calls in request order (InMemoryUniquenessProvider.kt:
 * 20-35).  Request t holds states [tx_state_begin[t], tx_state_begin[t+1]) (begin[0] == 0, monotone: CV_E_ARGS
 * otherwise), its id is tx_id[t], its caller caller[t].
 *   - tx_enable[t] == 0 (NULL: all enabled): the request is skipped; it commits nothing, conflicts with nothing,
 *     tx_status[t] = CV_UNIQ_SKIPPED.
 *   - A request conflicts iff one of its states is in the set when its turn comes: resident before the call, or
 *     put by an EARLIER ACCEPTED request of this batch.  It commits nothing; tx_status[t] = CV_UNIQ_CONFLICT,
 *     state_conflict[i] = 1 and consumed_id / consumed_index / consumed_caller[i] = the consuming record for each
 *     conflicting state i, state_conflict[i] = 0 and a zero record for its other states.
 *   - Otherwise tx_status[t] = CV_UNIQ_OK and every state is put with (tx_id[t], its index in the request,
 *     caller[t]); a state the request repeats is re-put, so the last index wins.  A request without states is
 *     accepted.  state_conflict and the records of skipped and accepted requests are zero. */
int cv_uniq_commit_batch(cv_uniq *u, size_t ntx, const uint8_t *state_key /* nstates*32 */,
                         const uint32_t *tx_state_begin /* ntx+1 */, const uint8_t *tx_id /* ntx*32 */,
                         const uint32_t *caller /* ntx */, const uint8_t *tx_enable /* ntx, NULL = all */,
                         uint8_t *tx_status /* ntx */, uint8_t *state_conflict /* nstates */,
                         uint8_t *consumed_id /* nstates*32 */, uint32_t *consumed_index /* nstates */,
                         uint32_t *consumed_caller /* nstates */);

/* committedStates[key] for n keys (InMemoryUniquenessProvider.kt:24; PersistentUniquenessProvider.kt:66): found[i]
 * = 1 and the consuming record, or 0 and a zero record.  Read-only. */
int cv_uniq_lookup(cv_uniq *u, size_t n, const uint8_t *state_key /* n*32 */, uint8_t *found /* n */,
                   uint8_t *consumed_id /* n*32 */, uint32_t *consumed_index /* n */, uint32_t *consumed_caller /* n */);

/* Warms the set from a durable log (the rows of PersistentUniquenessProvider's node_notary_commit_log,
 * PersistentUniquenessProvider.kt:30-49).  The keys must be distinct within the call and not resident:
 * otherwise CV_E_ARGS, the set unchanged (the check runs on the device before the first insert). */
int cv_uniq_load(cv_uniq *u, size_t n, const uint8_t *state_key /* n*32 */, const uint8_t *consumed_id /* n*32 */,
                 const uint32_t *consumed_index /* n */, const uint32_t *consumed_caller /* n */);

/* DistributedImmutableMap.snapshot (node/src/main/kotlin/net/corda/node/services/transactions/
 * DistributedImmutableMap.kt:87-92: every entry written out), in chunks of at most max_entries records: record j of a
 * call is (state_key[j], consumed_id[j], consumed_index[j], consumed_caller[j]), byte for byte what was committed.
 *   - cursor is opaque.  {0, 0} starts a pass; each call advances it; after the call that delivers the last entries
 *     cursor[0] == UINT64_MAX.  A call with such a finished cursor returns CV_OK with *n = 0 and writes no record.
 *   - A call writes *n <= max_entries records, and of the four arrays only the *n entries used: nothing before or
 *     behind them.  *n may be 0 on a call that is not the last (a stretch of empty slots): loop on the cursor, not on
 *     *n.  One call looks at max(2 * max_entries, 65,536) slots of the table at the most (2 x: the table is at most
 *     half full), so a pass with a small buffer takes about resident / max_entries calls.
 *   - Over one pass every resident entry is reported exactly once, within a call in ascending slot order.  Two passes
 *     over an unchanged set are byte-identical.  The order is the table's, not the order of commitment.
 *   - The set keeps an epoch that every call advances which may change the table's contents or layout:
 *     cv_uniq_commit_batch and cv_notarise_batch (also when they accepted nothing), cv_uniq_load, cv_uniq_install,
 *     cv_uniq_clear, and a cv_uniq_reserve that rehashes.  The cursor carries the epoch of the call that started the
 *     pass; continuing a pass after the epoch moved, or with a cursor no pass of this set gave, returns CV_E_ARGS and
 *     writes nothing: a torn snapshot is refused.  Lookup, stats and snapshot leave the epoch alone.
 *   - max_entries == 0 or a NULL cursor, n or array: CV_E_ARGS.  max_entries above 2^30: CV_E_TOO_LARGE.  A failed
 *     call writes nothing, *n and the cursor included. */
int cv_uniq_snapshot(cv_uniq *u, uint64_t cursor[2], size_t max_entries, uint8_t *state_key /* max_entries*32 */,
                     uint8_t *consumed_id /* max_entries*32 */, uint32_t *consumed_index /* max_entries */,
                     uint32_t *consumed_caller /* max_entries */, size_t *n);

/* map.clear() (DistributedImmutableMap.kt:98): afterwards the set is empty, CV_UNIQ_STAT_RESIDENT is 0, every key is
 * absent and may be committed again.  Capacity and slot count are kept. */
int cv_uniq_clear(cv_uniq *u);

/* DistributedImmutableMap.install (DistributedImmutableMap.kt:95-105): map.clear(), then put every entry of a
 * snapshot, as ONE step: afterwards the set holds exactly the n given entries, whatever it held before.  The new
 * contents are built in a fresh table beside the old one, which is swapped in on success, so a failed call leaves the
 * set exactly as it was: a key repeated within the call is CV_E_ARGS, n above 2^30 CV_E_TOO_LARGE, no memory for the
 * second table CV_E_OOM.  n == 0 is cv_uniq_clear.  The capacity becomes max(capacity, n); it never shrinks.  A Raft
 * state machine calls it from its one writer thread (Copycat's state machine thread). */
int cv_uniq_install(cv_uniq *u, size_t n, const uint8_t *state_key /* n*32 */, const uint8_t *consumed_id /* n*32 */,
                    const uint32_t *consumed_index /* n */, const uint32_t *consumed_caller /* n */);

/* The parallel decision rounds a commit runs at the most before one lane decides the requests still open in order
 * (0 = that serial tail only; at the most 64; default 8).  A batch without conflicts needs one round, a chain of k
 * requests each conflicting with the one before it k.  The result never depends on it: tests force each path. */
int cv_uniq_set_max_rounds(cv_uniq *u, int rounds);

/* Diagnostics: out[k] for k < nout (CV_UNIQ_STAT_*; entries past CV_UNIQ_STAT_COUNT are zero). */
#define CV_UNIQ_STAT_RESIDENT 0   /* states in the set */
#define CV_UNIQ_STAT_CAPACITY 1
#define CV_UNIQ_STAT_SLOTS 2
#define CV_UNIQ_STAT_ROUNDS 3     /* rounds the last commit ran */
#define CV_UNIQ_STAT_TAIL 4       /* requests the last commit's serial tail decided */
#define CV_UNIQ_STAT_PROBE 5      /* longest probe of the table in the last call, in slots */
#define CV_UNIQ_STAT_WRAPS 6      /* probes that passed the table's last slot, since open */
#define CV_UNIQ_STAT_COUNT 7
int cv_uniq_stats(cv_uniq *u, uint64_t *out, size_t nout);

/* tx_ok[t] = AND of verdict bits [tx_sig_begin[t], tx_sig_begin[t+1]); a transaction with no
 * signatures is not ok (SignedTransaction requires sigs.isNotEmpty(), SignedTransaction.kt:27-29). */
int cv_tx_verdicts(size_t ntx, const uint64_t *verdict_bitmap, const uint32_t *tx_sig_begin, uint8_t *tx_ok);

/* Missing signers: N x SignedTransaction.getMissingSignatures() (SignedTransaction.kt:89-93) with the verdict
 * verifySignatures (SignedTransaction.kt:58-72) draws from it, CompositeKey.isFulfilledBy (CompositeKey.kt:49, 75-81)
 * evaluated on the device for every mustSign entry of every transaction.
 *   Semantics, the reference's.  sigKeys = the set of the transaction's signer keys.  A Leaf is fulfilled iff its key
 *     is in sigKeys.  A Node is fulfilled iff the sum over its children of weights[i] where child i is fulfilled is >=
 *     threshold: the sum is a Kotlin Int (32-bit two's complement, it WRAPS), the compare signed.  The 0.7 constructor
 *     validates nothing: weights may be negative, a threshold <= 0 is fulfilled by nobody's signature, a Node without
 *     children is fulfilled iff threshold <= 0, a child listed twice counts twice.
 *   Key identity.  The call compares the 32 bytes it is given, all of them, and decodes nothing.  The reference
 *     compares EdDSAPublicKeys by getAbyte(), the canonical re-encoding, not by the wire bytes (the wire key
 *     ed ff .. ff 7f, y = p, re-encodes to 32 zero bytes).  The binding therefore passes getAbyte() for leaf keys and
 *     signer keys alike.
 *   Encoding.  The binding flattens each mustSign entry (a requirement) in post-order and concatenates them: node k
 *     has kind[k] (CV_CK_LEAF / CV_CK_NODE), a Leaf its key leaf_key[k][32] (zero for a Node), a Node threshold[k]
 *     (zero for a Leaf) and the children child[child_begin[k] .. child_begin[k+1]) (absolute node indices) with
 *     weight[] beside them; a Leaf's child range is empty and is not read.  Requirement r is nodes [req_begin[r],
 *     req_begin[r+1]), its root last; every child of node k lies in [req_begin[r], k).  A node may be the child of
 *     several nodes: the encoding is a DAG that evaluates as the tree it unfolds to, so equal subtrees may be shared.
 *     Transaction t owns requirements [tx_req_begin[t], tx_req_begin[t+1]) and the signer keys sig_key[tx_sig_begin[t]
 *     .. tx_sig_begin[t+1])[32]; tx_sig_begin is the array cv_verify_transactions takes.
 *   req_allowed[r] (NULL: none): non-zero when requirement r equals one of allowedToBeMissing.  CompositeKey equality
 *     is structural and stays with the binding (a set lookup; the reference's callers pass nothing or one notary key).
 *   verdict_bitmap (NULL: all valid): the verdict bits of the signatures, as cv_ed25519_verify_batch writes them.
 *   req_missing[r]: 0 fulfilled; 1 missing — getMissingSignatures as it stands, whatever req_allowed and the bitmap
 *     say; 2 malformed: a kind outside {0, 1}, a child range that descends or ends past nchild, a child index outside
 *     [req_begin[r], k), an empty requirement.  Whatever the child arrays hold, no kernel reads outside a
 *     requirement's own nodes or its transaction's own signer keys.  Equal requirements are each flagged.
 *   tx_status[t], first match wins: CV_VS_MALFORMED if one of its requirements is malformed; CV_VS_BAD_SIGNATURE if it
 *     has no signatures, or a bitmap is given and one of its bits is 0 (the rule of cv_tx_verdicts, and the
 *     reference's precedence: checkSignaturesAreValid runs before the missing check); CV_VS_MISSING if some
 *     req_missing[r] == 1 with req_allowed[r] == 0; else CV_VS_OK.  A transaction without requirements is never
 *     CV_VS_MISSING.  Duplicate signer keys count once (sigKeys is a set).
 *   wide_min: a transaction whose max(nodes, 1) x max(signers, 1) reaches it is decided by one wave (signer keys
 *     staged through the LDS) instead of one lane; 0 = the default (4096), 1 = always, UINT32_MAX = never.  The
 *     result never depends on it: tests force each path.  Either way the cost is nodes x signers first-word compares
 *     (no hashing): the binding bounds the size of a transaction.
 * Synchronous, on one device (the least loaded).  Before any device work: tx_req_begin, tx_sig_begin and req_begin
 * with begin[0] == 0, monotone, the last entry equal to its count, child_begin[0] == 0 and child_begin[nnodes] ==
 * nchild, no array missing that a non-zero count needs (CV_E_ARGS otherwise; what lies between child_begin's ends is
 * checked per requirement on the device, so a bad tree fails its transaction and not the batch); a count above
 * 0xfffffffe: CV_E_TOO_LARGE.  ntx == 0 returns CV_OK and writes nothing.  Outputs as under Conventions. */
#define CV_CK_LEAF 0
#define CV_CK_NODE 1
#define CV_VS_OK 0
#define CV_VS_BAD_SIGNATURE 1   /* no signatures, or (bitmap given) a signature's bit is 0 */
#define CV_VS_MISSING 2         /* SignaturesMissingException: a requirement missing and not allowed */
#define CV_VS_MALFORMED 3       /* a requirement of this transaction is not a tree encoding (no reference counterpart) */
int cv_missing_signers(cv_ctx *ctx, size_t ntx, size_t nreq, size_t nnodes, size_t nchild, size_t nsig,
                       const uint8_t *kind /* nnodes */, const uint8_t *leaf_key /* nnodes*32 */,
                       const int32_t *threshold /* nnodes */, const uint32_t *child_begin /* nnodes+1 */,
                       const uint32_t *child /* nchild */, const int32_t *weight /* nchild */,
                       const uint32_t *req_begin /* nreq+1 */, const uint32_t *tx_req_begin /* ntx+1 */,
                       const uint8_t *sig_key /* nsig*32 */, const uint32_t *tx_sig_begin /* ntx+1 */,
                       const uint8_t *req_allowed /* nreq, NULL = none */,
                       const uint64_t *verdict_bitmap /* ceil(nsig/64), NULL = all valid */, uint32_t wide_min,
                       uint8_t *req_missing /* nreq */, uint8_t *tx_status /* ntx */);
/* host only: the bytes of cv_missing_signers_device's d_workspace */
uint64_t cv_missing_signers_workspace(size_t ntx, size_t nnodes);

/* SignedTransaction.verifySignatures over a batch in one call (SignedTransaction.kt:59-71, 83-87 with
 * WireTransaction.id, WireTransaction.kt:45-52): the ids of ntx transactions (leaves as cv_merkle_tx_ids_ex) and
 * the verify of their signatures over those ids, the ids staying on the device as the messages.  The signatures
 * of transaction t are records [tx_sig_begin[t], tx_sig_begin[t+1]) of pk[][32] / sig[][64].
 *   tx_ok[t]      = 1 iff the transaction has at least one leaf, at least one signature, and every signature
 *                   verifies over its RECOMPUTED id (cv_merkle_tx_ids_ex + cv_ed25519_verify_batch over the ids +
 *                   cv_tx_verdicts, result for result).  The caller still compares ids with the claimed
 *                   SignedTransaction.id (line 70).  The accept/reject verdict is the reference's; the exception
 *                   is settled only for tx_ok == 1 with equal ids: for any other transaction the shim re-verifies
 *                   its signatures over the CLAIMED id (cv_ed25519_verify_batch), because the reference throws
 *                   the first bad signature's SignatureException before it compares ids.
 *   ids[ntx][32], tx_status[ntx] (CV_TX_OK / CV_TX_EMPTY), sig_status[nsig] (CV_SIG_*): optional (NULL).
 * Transactions are cut into contiguous ranges over the devices as cv_merkle_tx_ids_ex's; pinned inputs are
 * DMAed in place.  _async: ticket and cv_wait as cv_ed25519_verify_batch_async. */
int cv_verify_transactions(cv_ctx *ctx, size_t ntx, const uint8_t *leaf_arena, const uint64_t *leaf_off,
                           const uint32_t *leaf_len, const uint32_t *tx_leaf_begin /* ntx+1 */, const uint8_t *pk,
                           const uint8_t *sig, const uint32_t *tx_sig_begin /* ntx+1 */, uint8_t *ids,
                           uint8_t *tx_status, uint8_t *sig_status, uint8_t *tx_ok /* ntx */);
int cv_verify_transactions_async(cv_ctx *ctx, size_t ntx, const uint8_t *leaf_arena, const uint64_t *leaf_off,
                                 const uint32_t *leaf_len, const uint32_t *tx_leaf_begin, const uint8_t *pk,
                                 const uint8_t *sig, const uint32_t *tx_sig_begin, uint8_t *ids, uint8_t *tx_status,
                                 uint8_t *sig_status, uint8_t *tx_ok, uint64_t *ticket);
/* cv_verify_transactions (ticket NULL) or its _async form (ticket non-NULL) with the leaf arena's size, bounded as
 * cv_merkle_tx_ids_bounded: leaves past leaf_arena[leaf_arena_bytes) or wrapping give CV_E_ARGS before any read. */
int cv_verify_transactions_ex(cv_ctx *ctx, size_t ntx, const uint8_t *leaf_arena, uint64_t leaf_arena_bytes,
                              const uint64_t *leaf_off, const uint32_t *leaf_len, const uint32_t *tx_leaf_begin,
                              const uint8_t *pk, const uint8_t *sig, const uint32_t *tx_sig_begin, uint8_t *ids,
                              uint8_t *tx_status, uint8_t *sig_status, uint8_t *tx_ok, uint64_t *ticket);

/* The notary's commit step for a whole batch in ONE call: N x NotaryFlow.Service.call (core/src/main/kotlin/net/corda/
 * flows/NotaryFlow.kt:96-146) with, when `validating`, the signature checks of ValidatingNotaryFlow.beforeCommit
 * (ValidatingNotaryFlow.kt:24-45; SignedTransaction.kt:34-38 `tx`, 58-93 verifySignatures, checkSignaturesAreValid,
 * getMissingSignatures).  It is the composition of cv_merkle_tx_ids_bounded, cv_ed25519_verify_batch over the ids,
 * cv_missing_signers (with the verify's bitmap), cv_uniq_commit_batch and cv_ed25519_sign_keyed, result for result, with
 * the decisions between them made on the device: one upload, one read-back.  Contract verification and dependency
 * resolution stay out of scope, as for the calls it is made of.
 *   Transactions.  Leaves as cv_merkle_tx_ids_bounded (tx_leaf_begin[0] == 0, monotone; a leaf past
 *     leaf_arena[leaf_arena_bytes), or one whose off + len wraps: CV_E_ARGS before any read).  claimed_id[t] is
 *     SignedTransaction.id, caller[t] the requesting party's handle (cv_uniq), tx_pre[t] non-zero when the host's
 *     TimestampChecker found the timestamp invalid (the leaves are not decoded here).
 *   State keys.  The states of transaction t are its first tx_input_count[t] leaves (inputs come first in
 *     WireTransaction's leaf order); a state's key is that leaf's SHA-256 digest, the documented key of cv_uniq, taken
 *     from the leaf hashes the id is built from: not hashed again and not uploaded.  nstates = the sum of
 *     tx_input_count; state i of the outputs counts the states of the transactions in order.  tx_input_count[t] above
 *     the transaction's leaf count: CV_E_ARGS.
 *   outcome[t], first match wins, in the reference's order:
 *     1. CV_NS_EMPTY, then CV_NS_ID_MISMATCH: `val wtx = stx.tx` (NotaryFlow.kt:99) recomputes the id and checks it
 *        against the claimed one OUTSIDE the try, so either fails the flow instead of answering with a NotaryError.
 *     2. CV_NS_TIMESTAMP_INVALID: validateTimestamp (NotaryFlow.kt:102,115-119), tx_pre.
 *     3. validating only (a non-validating notary's beforeCommit is empty, NotaryFlow.kt:129-131: it commits
 *        transactions with bad signatures).  checkSignaturesAreValid (SignedTransaction.kt:82-87) throws at the FIRST
 *        signature, in order, that fails — here: sig_pre[i] != 0 or a zero verdict bit — and that signature settles
 *        the class: CV_NS_BAD_KEY (InvalidKeyException, re-thrown by ValidatingNotaryFlow.kt:34: the flow fails) when
 *        sig_pre[i] == 2, or sig_pre[i] == 0 and the device status is CV_SIG_BAD_KEY; CV_NS_TX_INVALID
 *        (SignatureException -> NotaryError.TransactionInvalid) otherwise.  A transaction without signatures is
 *        CV_NS_TX_INVALID, the rule of cv_tx_verdicts.  Then the missing-signers verdict of cv_missing_signers over
 *        the same batch (default wide_min; req_allowed honoured, duplicate signer keys counted once): CV_NS_MALFORMED,
 *        CV_NS_SIGNATURES_MISSING (req_missing says which).
 *     4. CV_NS_CONFLICT or CV_NS_SUCCESS from the uniqueness set, for the transactions that passed everything above,
 *        and only for those.
 *   The signatures are verified over the RECOMPUTED id, which stays on the device as the message.  A transaction that
 *     reaches step 3 has recomputed id == claimed id, so this is the reference's verify over the claimed id
 *     (SignedTransaction.kt:85) for every transaction whose signatures decide anything.
 *   first_bad[t] (optional): the absolute index of the signature that settled CV_NS_TX_INVALID / CV_NS_BAD_KEY,
 *     0xffffffff for every other transaction (one without signatures included, and all when not validating).
 *   req_missing (optional): cv_missing_signers' req_missing for every requirement of the batch, whatever the outcome.
 *   The commit is cv_uniq_commit_batch's, result for result, with tx_enable[t] = (nothing of steps 1-3 matched) and
 *     tx_id = the id: decided as sequential commits in request order; a gated-out transaction commits nothing and
 *     conflicts with nothing; state_conflict and consumed_* are that call's (zero for states without a conflict, and
 *     for every state of a transaction that is not CV_NS_CONFLICT); CV_E_OOM before any change and any output when
 *     resident + nstates > capacity.  Durability stays with the binding: it appends the accepted rows to its log
 *     before it releases a signature.
 *   notary_sig[t] = cv_ed25519_sign_keyed(s) over the 32 id bytes when outcome[t] == CV_NS_SUCCESS, 64 zero bytes
 *     otherwise.  The signing kernel runs for the accepted transactions alone: a signature over the id of a
 *     transaction that was not committed reaches no host-visible buffer.  Conflict reports (e.error.serialize() and
 *     sign(conflictData), NotaryFlow.kt:136-139) stay with the binding: it serialises them from the records and signs
 *     them with cv_ed25519_sign_keyed.
 *   Not validating: pk .. sig_pre and nreq .. req_allowed are ignored and may be NULL / 0; first_bad is all
 *     0xffffffff, req_missing is not written (there are no requirements).
 * Synchronous, on the set's device, serialised on the set's mutex; `u` and `s` must belong to `ctx` (CV_E_ARGS).
 * Before any device work: the range arrays as the component calls check them (begin[0] == 0, monotone, tx_req_begin
 * ends at nreq, req_begin at nnodes, child_begin[0] == 0 and child_begin[nnodes] == nchild), no array missing that a
 * non-zero count needs: CV_E_ARGS; a count above 0xfffffffe, or more than 2^30 transactions or states:
 * CV_E_TOO_LARGE.  ntx == 0 returns CV_OK and touches nothing.  Outputs as under Conventions. */
#define CV_NS_SUCCESS            0  /* committed; notary_sig[t] = signature over the id                      */
#define CV_NS_EMPTY              1  /* no leaves: MerkleTreeException, the flow fails                        */
#define CV_NS_ID_MISMATCH        2  /* recomputed id != claimed id: IllegalStateException, the flow fails    */
#define CV_NS_TIMESTAMP_INVALID  3  /* NotaryError.TimestampInvalid                                          */
#define CV_NS_TX_INVALID         4  /* first bad signature is a SignatureException: TransactionInvalid       */
#define CV_NS_BAD_KEY            5  /* first bad signature is an InvalidKeyException: the flow fails         */
#define CV_NS_SIGNATURES_MISSING 6  /* NotaryError.SignaturesMissing (req_missing says which)                */
#define CV_NS_MALFORMED          7  /* a requirement is not a tree encoding (CV_VS_MALFORMED)                */
#define CV_NS_CONFLICT           8  /* NotaryError.Conflict (state_conflict / consumed_* say with what)      */
int cv_notarise_batch(cv_ctx *ctx, cv_uniq *u, const cv_signer *s, int validating, size_t ntx,
    /* transactions: leaves as cv_merkle_tx_ids_bounded */
    const uint8_t *leaf_arena, uint64_t leaf_arena_bytes, const uint64_t *leaf_off, const uint32_t *leaf_len,
    const uint32_t *tx_leaf_begin /* ntx+1 */, const uint32_t *tx_input_count /* ntx */,
    const uint8_t *claimed_id /* ntx*32 */, const uint32_t *caller /* ntx */,
    const uint8_t *tx_pre /* ntx, NULL = none: non-zero = the host's TimestampChecker said invalid */,
    /* signatures (validating only; ignored and may be NULL otherwise) */
    const uint8_t *pk /* nsig*32 */, const uint8_t *sig /* nsig*64 */, const uint32_t *tx_sig_begin /* ntx+1 */,
    const uint8_t *sig_pre /* nsig, NULL = none: 1 = host prefilter SignatureException (bad length),
                                                  2 = host prefilter InvalidKeyException (not EdDSA) */,
    /* mustSign requirements, exactly the arrays of cv_missing_signers (validating only) */
    size_t nreq, size_t nnodes, size_t nchild, const uint8_t *kind, const uint8_t *leaf_key,
    const int32_t *threshold, const uint32_t *child_begin, const uint32_t *child, const int32_t *weight,
    const uint32_t *req_begin, const uint32_t *tx_req_begin, const uint8_t *sig_key, const uint8_t *req_allowed,
    /* outputs */
    uint8_t *outcome /* ntx */, uint8_t *ids /* ntx*32, optional */, uint8_t *notary_sig /* ntx*64 */,
    uint32_t *first_bad /* ntx, optional: absolute index of the first failing signature, 0xffffffff = none */,
    uint8_t *req_missing /* nreq, optional */, uint8_t *state_conflict /* nstates */,
    uint8_t *consumed_id /* nstates*32 */, uint32_t *consumed_index /* nstates */,
    uint32_t *consumed_caller /* nstates */);

/* N x FilteredTransaction.verify(merkleRoot) (MerkleTransaction.kt:173-178 with PartialMerkleTree.kt:118-144) from
 * the tear-offs' leaf BLOBS: the verifier's counterpart of cv_filtered_build.  The check list of tree t —
 * FilteredLeaves.getFilteredHashes(), MerkleTransaction.kt:112-117 — is the SHA-256 digests of its filtered leaves,
 * computed on the device by the leaf kernel of cv_merkle_tx_ids; they are never uploaded and never hashed on the host.
 *   - verdict[t] and status[t] (optional) are cv_partial_merkle_verify's over those digests, result for result.
 *   - A tear-off with no filtered leaves gets verdict 0 and status CV_PMT_NO_INCLUDED: the reference tests
 *     `hashes.size == 0` (:175-176) before it touches the tree, so this wins over CV_PMT_MALFORMED.
 * Synchronous, on one device (the least loaded).  All before any device work: the ranges as
 * cv_partial_merkle_verify's for tree_begin and the same rules for tx_leaf_begin (begin[0] == 0, monotone, the end
 * equals the count: CV_E_ARGS otherwise); a leaf past leaf_arena[leaf_arena_bytes), or whose off + len wraps, is
 * CV_E_ARGS; more than 0xfffffffe tear-offs, leaves or nodes CV_E_TOO_LARGE; ntx == 0 returns CV_OK and touches
 * nothing; a NULL context is checked last. */
#define CV_PMT_NO_INCLUDED 4   /* MerkleTreeException("Transaction without included leaves.") */
int cv_filtered_verify(cv_ctx *ctx, size_t ntx,
    /* the FILTERED leaves of tear-off t, serialised, in getFilteredHashes order (inputs, outputs, attachments,
       commands): blobs as cv_merkle_tx_ids_bounded takes them */
    const uint8_t *leaf_arena, uint64_t leaf_arena_bytes, const uint64_t *leaf_off, const uint32_t *leaf_len,
    const uint32_t *tx_leaf_begin /* ntx+1 */,
    /* the partial trees, exactly the arrays of cv_partial_merkle_verify / the outputs of cv_filtered_build */
    size_t nnodes, const uint8_t *kind, const uint32_t *left, const uint32_t *right,
    const uint8_t *node_hash /* nnodes*32 */, const uint32_t *tree_begin /* ntx+1 */,
    const uint8_t *root /* ntx*32 */, uint8_t *verdict /* ntx */, uint8_t *status /* ntx, optional */);

/* N x NodeInterestRates.Oracle.sign(ftx, merkleRoot) (samples/irs-demo/src/main/kotlin/net/corda/irs/api/
 * NodeInterestRates.kt:190-225; the client is RatesFixFlow.kt:100-110) in one call: the tear-off verified as
 * cv_filtered_verify does, the oracle's refusals in the reference's order, the root signed with the service's fixed
 * key.  The binding decodes the leaves (Kryo stays on the JVM) and passes one byte per filtered leaf, leaf_pre:
 *   0 fine; 1 not a command — an input, output or attachment (the require at :197); 2 a command the service does not
 *   vouch for — not a Fix, or the oracle is not among its signers (:199-205); 3 a command it vouches for whose data
 *   it does not know, or knows differently (UnknownFix, :213-217).  Any other value: CV_E_ARGS before any device work.
 * outcome[t], first match wins:
 *   CV_TS_NO_LEAVES, CV_TS_MALFORMED, CV_TS_VERIFY_FAILED from the verify (its status CV_PMT_NO_INCLUDED,
 *   CV_PMT_MALFORMED, its verdict 0); then CV_TS_NOT_COMMANDS, CV_TS_WRONG_COMMAND, CV_TS_UNKNOWN for the LOWEST class
 *   of leaf_pre present among the tear-off's leaves — each of the reference's tests looks at every leaf before the
 *   next one runs; CV_TS_SUCCESS otherwise.  The reference's `fixes.isEmpty()` branch (:208-209) cannot be reached:
 *   past the first tests there is at least one leaf and every leaf is a command the service vouches for.
 * first_bad[t] (optional): for CV_TS_NOT_COMMANDS / WRONG_COMMAND / UNKNOWN the absolute index of the first filtered
 *   leaf of the deciding class (the reference names the first unknown fix in order); 0xffffffff for every other outcome.
 * sig_out[t] = cv_ed25519_sign_keyed(s) over the 32 bytes of root[t] when outcome[t] == CV_TS_SUCCESS, bit for bit —
 *   signingKey.signWithECDSA(merkleRoot.bytes, identity), :224 — and 64 zero bytes otherwise.  The signing kernel
 *   runs for the accepted tear-offs alone: a signature over a refused root reaches no host-visible buffer.
 * s must belong to ctx.  Synchronous, on one device (the least loaded); one upload, two synchronisations (the
 * accepted count, the read-back).  Argument checks as cv_filtered_verify. */
#define CV_TS_SUCCESS        0  /* sig_out[t] = signature over root[t]                                        */
#define CV_TS_NO_LEAVES      1  /* MerkleTreeException out of ftx.verify (MerkleTransaction.kt:175-176)       */
#define CV_TS_MALFORMED      2  /* the nodes are not a tree encoding: the shim throws IllegalArgumentException */
#define CV_TS_VERIFY_FAILED  3  /* MerkleTreeException("... Couldn't verify partial Merkle tree.") (:191-193) */
#define CV_TS_NOT_COMMANDS   4  /* some leaf_pre == 1: IllegalArgumentException (the require at :197)         */
#define CV_TS_WRONG_COMMAND  5  /* some leaf_pre == 2: IllegalArgumentException (:204-205)                    */
#define CV_TS_UNKNOWN        6  /* some leaf_pre == 3: UnknownFix of leaf first_bad[t] (:213-217)             */
int cv_tearoff_sign_batch(cv_ctx *ctx, const cv_signer *s, size_t ntx,
    /* the filtered leaves and the partial trees: the inputs of cv_filtered_verify */
    const uint8_t *leaf_arena, uint64_t leaf_arena_bytes, const uint64_t *leaf_off, const uint32_t *leaf_len,
    const uint32_t *tx_leaf_begin /* ntx+1 */, size_t nnodes, const uint8_t *kind, const uint32_t *left,
    const uint32_t *right, const uint8_t *node_hash /* nnodes*32 */, const uint32_t *tree_begin /* ntx+1 */,
    const uint8_t *root /* ntx*32 */,
    const uint8_t *leaf_pre /* nleaves, NULL = none: the service's verdict on each filtered leaf's CONTENT */,
    uint8_t *outcome /* ntx */, uint32_t *first_bad /* ntx, optional */, uint8_t *sig_out /* ntx*64 */);

/* The body of ResolveTransactionsFlow.call (core/src/main/kotlin/net/corda/flows/ResolveTransactionsFlow.kt:96-111)
 * over the ntx transactions downloadDependencies returned, in ONE call.  The transactions are given in DOWNLOAD ORDER,
 * the order of resultQ.values (:150,:170): topologicalSort's result depends on it.  The binding decodes the StateRefs
 * (Kryo stays on the JVM) and passes, per input, its txhash and index, and per transaction its number of outputs; the
 * leaves are not decoded here.
 *   :39-45  forwardGraph: input_dep[i] = the transaction of the batch whose CLAIMED id (stx.id, the key of resultQ)
 *           equals input_txhash[i], or 0xffffffff: not in the batch — by construction of downloadDependencies
 *           (:158-174) a transaction the node already stores; that lookup stays with the binding.
 *   :167,:41 `stx.tx` of every download is touched before anything is verified: one transaction that is CV_RS_EMPTY or
 *           CV_RS_ID_MISMATCH fails the flow as a whole, graph[CV_RG_STATUS] = CV_RG_BAD_ID.
 *   :170,:65 check(putIfAbsent == null), require(result.size == transactions.size): two transactions with one id,
 *           CV_RG_DUPLICATE_ID.  CV_RG_BAD_ID takes precedence: the download rounds, which are not an input here,
 *           could meet the two in either order, and both fail the flow.
 *   :37-67  topologicalSort: order[] is its result, element for element (the dependents of a transaction distinct and
 *           in download order, the LinkedHashSet of :43; visit in download order; post-order, reversed).
 *   :105-111 the walk over order: stx.toLedgerTransaction(serviceHub) is verifySignatures() WITHOUT allowed keys
 *           (SignedTransaction.kt:134 -> :58-72: checkSignaturesAreValid, then the missing signers), then every input
 *           through loadState (ServiceHub.kt:46-49), in order: a dependency in the batch that was not recorded before
 *           — it does not stand earlier in order; only a self-reference or a cycle of hand-fed input_txhash gets
 *           there — is a TransactionResolutionException, CV_RS_UNRESOLVED; one that was, with
 *           tx_output_count[dep] <= input_index, makes `outputs[stateRef.index]` throw, CV_RS_BAD_INPUT.  The walk
 *           stops at the first transaction that fails.  ltx.verify() (:108, the contracts) and recordTransactions
 *           (:109) are NOT run here: the binding runs them for the graph[CV_RG_N_PASS] leading transactions of order.
 *   :119-125 the final single stx / wtx is one transaction that is not recorded; it stays with the binding.
 * outcome[t], the verdict of transaction t on its own, whatever the order; first match wins:
 *     1. CV_RS_EMPTY, CV_RS_ID_MISMATCH                 as CV_NS_*
 *     2. CV_RS_TX_INVALID, CV_RS_BAD_KEY                the FIRST failing signature in order settles the class, as in
 *        cv_notarise_batch (sig_pre likewise); no signatures at all is CV_RS_TX_INVALID, the rule of cv_tx_verdicts
 *        (the reference cannot construct one, SignedTransaction.kt:28).  Signatures are verified over the id
 *        recomputed on the device: past class 1 it equals the claimed id the reference verifies over.
 *     3. CV_RS_MALFORMED, CV_RS_SIGNATURES_MISSING      cv_missing_signers over the same batch, nothing allowed
 *     4. CV_RS_BAD_INPUT                                some input of t refers to a transaction of the batch with
 *        tx_output_count <= input_index; bad_input[t] = the absolute index of the first such input
 *     5. CV_RS_OK
 *   first_bad[t], req_missing[r] (optional): as cv_notarise_batch.  bad_input[t]: 0xffffffff unless CV_RS_BAD_INPUT.
 *   input_status[i]: 0 external, 1 in the batch and in range, 2 in the batch and out of range.
 * graph[CV_RG_WORDS]:
 *   CV_RG_STATUS     CV_RG_OK, CV_RG_BAD_ID or CV_RG_DUPLICATE_ID
 *   CV_RG_WHICH      the smallest index of a transaction that is EMPTY / ID_MISMATCH, respectively the smallest index
 *                    of a transaction whose id occurs more than once; 0xffffffff with CV_RG_OK
 *   CV_RG_N_PASS     the leading transactions of order that pass everything this call checks (ntx: all of them)
 *   CV_RG_STOP_CLASS, CV_RG_STOP_TX, CV_RG_STOP_INPUT   what stopped the walk: the outcome of the transaction it
 *                    stopped at (with its bad_input), or CV_RS_UNRESOLVED / CV_RS_BAD_INPUT with the input met, going
 *                    through the transaction's inputs in order (an unresolved input is met before an out-of-range
 *                    one that comes later); 0xffffffff each when nothing stopped it
 *   CV_RG_EXTERNAL   the number of inputs of status 0
 *   CV_RG_MAXPROBE, CV_RG_WRAPS   diagnostics of the join table (longest probe, probes past its last slot)
 *   With CV_RG_STATUS != CV_RG_OK, order is zero-filled, N_PASS is 0 and STOP_* are 0xffffffff; with several
 *   transactions of one id, input_dep names the smallest index among them.
 * seed: of the join table's hash (ids are hashes the serving peer can grind, so all eight words are mixed with it and
 * no id bits choose a slot directly); 0 draws a fresh one, any other value makes a run reproducible.  The results
 * but CV_RG_MAXPROBE / CV_RG_WRAPS do not depend on it.
 * Synchronous, on one device (the least loaded); one upload, one read-back; order and the walk are computed on the
 * host after it (a lexicographic depth-first order is sequential).  All before any device work: the range arrays
 * (begin[0] == 0, monotone, the last entry the count) and child_begin's ends malformed, a leaf past
 * leaf_arena[leaf_arena_bytes) or whose off + len wraps, or a missing array that a non-zero count needs: CV_E_ARGS;
 * a count above 0xfffffffe, or more than 2^30 transactions or inputs: CV_E_TOO_LARGE; ntx == 0 returns CV_OK and
 * touches nothing; ninputs == 0 is legal; a NULL context is checked last.  A probe that runs out of slots (it cannot):
 * CV_E_HIP.  With CV_OPT_TIMELINE = 1 the call times its stages with HIP events (CV_STATS_RESOLVE).  Outputs as under
 * Conventions. */
#define CV_RS_OK                 0
#define CV_RS_EMPTY              1  /* no leaves: MerkleTreeException out of stx.tx                          */
#define CV_RS_ID_MISMATCH        2  /* recomputed id != claimed id: IllegalStateException                    */
#define CV_RS_TX_INVALID         4  /* first bad signature is a SignatureException                           */
#define CV_RS_BAD_KEY            5  /* first bad signature is an InvalidKeyException                         */
#define CV_RS_SIGNATURES_MISSING 6  /* SignaturesMissingException (req_missing says which)                   */
#define CV_RS_MALFORMED          7  /* a requirement is not a tree encoding (CV_VS_MALFORMED)                */
#define CV_RS_BAD_INPUT          9  /* outputs[stateRef.index] out of range: IndexOutOfBoundsException       */
#define CV_RS_UNRESOLVED        10  /* CV_RG_STOP_CLASS only: TransactionResolutionException                 */
#define CV_RG_OK 0
#define CV_RG_BAD_ID 1
#define CV_RG_DUPLICATE_ID 2
#define CV_RG_STATUS 0
#define CV_RG_WHICH 1
#define CV_RG_N_PASS 2
#define CV_RG_STOP_CLASS 3
#define CV_RG_STOP_TX 4
#define CV_RG_STOP_INPUT 5
#define CV_RG_EXTERNAL 6
#define CV_RG_MAXPROBE 7
#define CV_RG_WRAPS 8
#define CV_RG_WORDS 9
int cv_resolve_batch(cv_ctx *ctx, size_t ntx,
    /* transactions and signatures, exactly as cv_notarise_batch (always validating) */
    const uint8_t *leaf_arena, uint64_t leaf_arena_bytes, const uint64_t *leaf_off, const uint32_t *leaf_len,
    const uint32_t *tx_leaf_begin /* ntx+1 */, const uint8_t *claimed_id /* ntx*32 */,
    const uint8_t *pk /* nsig*32 */, const uint8_t *sig /* nsig*64 */, const uint32_t *tx_sig_begin /* ntx+1 */,
    const uint8_t *sig_pre /* nsig, NULL = none */,
    /* mustSign requirements, exactly the arrays of cv_missing_signers (no req_allowed) */
    size_t nreq, size_t nnodes, size_t nchild, const uint8_t *kind, const uint8_t *leaf_key,
    const int32_t *threshold, const uint32_t *child_begin, const uint32_t *child, const int32_t *weight,
    const uint32_t *req_begin, const uint32_t *tx_req_begin, const uint8_t *sig_key,
    /* the graph: the StateRefs of every transaction's inputs, in order, and its number of outputs */
    size_t ninputs, const uint32_t *tx_input_begin /* ntx+1 */, const uint8_t *input_txhash /* ninputs*32 */,
    const uint32_t *input_index /* ninputs */, const uint32_t *tx_output_count /* ntx */, uint64_t seed,
    /* outputs */
    uint8_t *outcome /* ntx */, uint32_t *first_bad /* ntx, optional */, uint8_t *req_missing /* nreq, optional */,
    uint32_t *bad_input /* ntx */, uint32_t *input_dep /* ninputs */, uint8_t *input_status /* ninputs */,
    uint32_t *order /* ntx */, uint32_t *graph /* CV_RG_WORDS */, uint8_t *ids /* ntx*32, optional */);

/* ---------------------------------------------------------------- the key store (the node's own signing)
 * KeyManagementService (core/src/main/kotlin/net/corda/core/node/services/Services.kt:189-219) as
 * PersistentKeyManagementService keeps it (node/src/main/kotlin/net/corda/node/services/keys/
 * PersistentKeyManagementService.kt:40-66): keys: Map<PublicKey, PrivateKey>, freshKey(), toPrivate(pk) — on one
 * device of the context, holding the EXPANDED private keys (a | prefix | Abyte, the 96 bytes of a cv_signer record)
 * addressed by public key, so that a spending node signs a batch in which every record names its own key
 * (CashFlow.kt:39-47, TwoPartyTradeFlow.kt:227-235,250, TwoPartyDealFlow.kt:254) without a key expansion per
 * signature and without handing a seed across the ABI per signature.
 *   - The identity of a key is its 32 encoded bytes.  No single key is deleted (the reference's map never removes
 *     one); cv_keystore_close overwrites the table before it frees it, and so does the rehash of
 *     cv_keystore_reserve with the table it replaces.
 *   - No entry point ever returns a, prefix or a seed, and there is no snapshot: the binding keeps the seeds durable
 *     (PersistentKeyManagementService's table) and warms a new store with cv_keystore_add.
 *   - Side channels: as cv_signer — the scalar multiplication selects table entries by secret digits; nothing
 *     else here branches on, or indexes by, secret data.
 *   - Calls on one store serialise on a mutex in the store (the reference's ThreadBox); the store has its own stream
 *     and workspace, so they take no device lock.  A store is closed before its context; cv_keystore_close(NULL) is
 *     a no-op.
 *   - Counts: n == 0 (ntx == 0) returns CV_OK and touches nothing; more than 0xfffffffe records: CV_E_TOO_LARGE; so
 *     is a capacity, or one call, of more than 2^30 keys.  A NULL store, context or required array: CV_E_ARGS.  All
 *     before any device work.  Outputs as under Conventions. */
typedef struct cv_keystore cv_keystore;
#define CV_KS_ADDED 0
#define CV_KS_PRESENT 1
#define CV_KS_OK 0
#define CV_KS_NO_KEY 1
int cv_keystore_open(cv_ctx *ctx, int device, size_t capacity_keys, cv_keystore **out);
void cv_keystore_close(cv_keystore *ks);
/* Room for capacity_keys keys: a rehash on the device into a table of at least twice as many slots; never shrinks. */
int cv_keystore_reserve(cv_keystore *ks, size_t capacity_keys);

/* N x (entropyToKeyPair / generateKeyPair, CryptoUtilities.kt:117-130) + keys[public] = private
 * (PersistentKeyManagementService.kt:53-61): seed[i] is expanded on the device, pk_out[i] = its public key, written
 * for every record, and status[i] = CV_KS_ADDED or CV_KS_PRESENT.  Of several records of one call with the same public
 * key the FIRST in index order is CV_KS_ADDED; a key already resident is CV_KS_PRESENT and its record is untouched.
 * The seeds go up through pinned staging that is wiped before the call returns; the device copy is cleared behind the
 * expansion.  A call that would take the store past its capacity (resident + n, repeats included) returns CV_E_OOM
 * before any change and any output. */
int cv_keystore_add(cv_keystore *ks, size_t n, const uint8_t *seed /* n*32 */, uint8_t *pk_out /* n*32 */,
                    uint8_t *status /* n */);

/* keys.contains(pk) for n keys (PersistentKeyManagementService.kt:51): found[i] = 1 or 0.  Read-only. */
int cv_keystore_contains(cv_keystore *ks, size_t n, const uint8_t *pk /* n*32 */, uint8_t *found /* n */);

/* N x KeyPair(pk, toPrivate(pk)).signWithECDSA(msg) (Services.kt:206-212, CryptoUtilities.kt:63-73): record i is signed
 * with ITS OWN key pk[i]; bit for bit cv_ed25519_sign_batch's signature with that key's seed.  A record whose key is
 * absent (toPrivate's IllegalStateException) gets status CV_KS_NO_KEY and 64 zero bytes; the others are signed
 * regardless.  A record past msg_arena[msg_arena_bytes), or whose off + len wraps: CV_E_ARGS before any copy. */
int cv_keystore_sign(cv_keystore *ks, size_t n, const uint8_t *pk /* n*32 */, const uint8_t *msg_arena,
                     uint64_t msg_arena_bytes, const uint64_t *msg_off, const uint32_t *msg_len,
                     uint8_t *sig_out /* n*64 */, uint8_t *status /* n */);

/* Diagnostics: out[k] for k < nout (entries past CV_KS_STAT_COUNT are zero). */
#define CV_KS_STAT_RESIDENT 0
#define CV_KS_STAT_CAPACITY 1
#define CV_KS_STAT_SLOTS 2
#define CV_KS_STAT_PROBE 3        /* longest probe of the table in the last call, in slots */
#define CV_KS_STAT_COUNT 4
int cv_keystore_stats(cv_keystore *ks, uint64_t *out, size_t nout);

/* The builder's signing step for a batch (TransactionBuilder.kt:93-98,132-141 under the flows' loops, CashFlow.kt:39-47):
 * ids from the leaves (as cv_merkle_tx_ids_bounded; they stay on the device as the messages), then transaction t is
 * signed by keys pk[tx_sig_begin[t] .. tx_sig_begin[t+1]) of the store, sig_out[j] = key j's signature over ids[t].
 * The keys are walked in order; the first index j (within the transaction) at which something fails settles
 * tx_status[t] and first_bad[t]:
 *   CV_ST_NO_KEY          key j is not in the store (IllegalStateException, CashFlow.kt:43 / Services.kt:210)
 *   CV_ST_ALREADY_SIGNED  key j equals an earlier key of the transaction (TransactionBuilder.kt:94); the scan of the
 *                         earlier keys is quadratic in ONE transaction's signer count
 *   CV_ST_EMPTY           no leaves (MerkleTreeException inside the first signWith: only at j = 0, after the two
 *                         checks above); a transaction with no leaves and no keys is CV_ST_EMPTY with first_bad 0
 * Otherwise CV_ST_OK with first_bad 0xffffffff (a transaction with leaves and no keys included).  A transaction that
 * is not CV_ST_OK is abandoned: all of its sig_out are 64 zero bytes; its id is still written (zero for no leaves).
 * Both range arrays start at 0, are monotone and end at their counts (tx_sig_begin[ntx] == nsig), a leaf past
 * leaf_arena[leaf_arena_bytes) or wrapping: CV_E_ARGS before any device work; `ks` must belong to `ctx`. */
#define CV_ST_OK 0
#define CV_ST_NO_KEY 1
#define CV_ST_ALREADY_SIGNED 2
#define CV_ST_EMPTY 3
int cv_sign_transactions(cv_ctx *ctx, cv_keystore *ks, size_t ntx,
    const uint8_t *leaf_arena, uint64_t leaf_arena_bytes, const uint64_t *leaf_off, const uint32_t *leaf_len,
    const uint32_t *tx_leaf_begin /* ntx+1 */,
    size_t nsig, const uint8_t *pk /* nsig*32 */, const uint32_t *tx_sig_begin /* ntx+1 */,
    uint8_t *tx_status /* ntx */, uint8_t *ids /* ntx*32 */, uint8_t *sig_out /* nsig*64 */,
    uint32_t *first_bad /* ntx, optional */);

/* ---------------------------------------------------------------- device-resident API
 * All pointers are device pointers on HIP device `device` (which must be in the context); work is
 * enqueued on `stream` (a hipStream_t, NULL = the context's stream for that device) and the call
 * returns without synchronising.  These are the entry points bench.py times (inputs resident in HBM).
 * A large batch may internally run part of its work on a per-device helper stream of the engine (the
 * drain overlap); `stream` waits on that work before anything the caller
 * enqueues after the call, so completion is still stream-ordered on `stream`.
 * Calls may use different streams, from any thread: the engine orders every use of a device's shared
 * verify workspace and key pool (a call on a new stream first waits for the previous call's work on
 * that workspace), so concurrent calls serialise on the device instead of racing.
 * Alignment (the kernels' vector accesses need it; a pointer below it faults the GPU, nothing checks it):
 *     16 bytes  d_pk, d_sig, d_keys, d_seed (inputs and outputs: records are read and written as 16-byte vectors),
 *               d_ids, d_workspace, d_leaf_key, d_sig_key
 *      8 bytes  d_bitmap (whole 64-bit words, 64-bit atomics), d_off, d_leaf_off
 *      4 bytes  d_len, d_leaf_len, d_key_index, d_tx_leaf_begin, and the 32-bit arrays of cv_missing_signers_device
 *               (d_threshold, d_child_begin, d_child, d_weight, d_req_begin, d_tx_req_begin, d_tx_sig_begin)
 *      none     d_status, d_tx_status, d_arena (messages and leaves may start at any byte; the engine reads the
 *               aligned 32-bit words that hold their bytes, never a word that holds none), d_kind, d_req_allowed,
 *               d_req_missing
 * Outputs as under Conventions: any prior contents, zero tail bits in d_bitmap, ceil(n/64) * 8 bytes of it written
 * and not one more, a zero id for an empty transaction; n == 0 (ntx == 0) enqueues nothing.
 */
int cv_ed25519_verify_device(cv_ctx *ctx, int device, size_t n, const void *d_pk, const void *d_sig,
                             const void *d_arena, const void *d_off, const void *d_len, void *d_bitmap,
                             void *d_status, void *stream);

/* Measurement entry point (bench.py): as cv_ed25519_verify_device (no status), but synchronous,
 * whole-chunk launches only (no drain overlap), and fills phase_ms[0..2] with the summed durations
 * of the verify kernels measured with HIP events on the launch stream.  Half-size schedule (default),
 * batches above 32,768: scalars (challenge hash, effective S, lattice, window digits) | points
 * (decode A and R, both odd-multiple tables) | hs_straus (multi-scalar multiplication + verdict
 * bits).  Batches up to 32,768 (latency forms): scalars and point pairs in one launch | bitmap clear |
 * tri-chain (<= 4,096) or quad Straus.  Full-width schedule: prep | Straus | finish (batched
 * inversion, encode, compare, bitmap). */
int cv_ed25519_verify_device_timed(cv_ctx *ctx, int device, size_t n, const void *d_pk, const void *d_sig,
                                   const void *d_arena, const void *d_off, const void *d_len, void *d_bitmap,
                                   void *stream, float *phase_ms);

/* Keyed device-resident batch: d_keys[nkeys][32], d_key_index[n] (uint32), the rest as
 * cv_ed25519_verify_device.  The nkeys key records are copied to the host (32 B each) to resolve
 * them against the key pool; new keys' tables are computed on `stream` before the verify.  Keyed
 * calls on one device must share one stream (the pool is reused across calls in stream order).
 * phase_ms NULL: returns without synchronising; else the call is synchronous and fills
 * phase_ms[0..3] = key tables, hash, comb, finish kernel durations (HIP events). */
int cv_ed25519_verify_device_keyed(cv_ctx *ctx, int device, size_t n, size_t nkeys, const void *d_keys,
                                   const void *d_key_index, const void *d_sig, const void *d_arena, const void *d_off,
                                   const void *d_len, void *d_bitmap, void *d_status, void *stream, float *phase_ms);

/* The distinct keys of d_pk[n][32], found on the device: d_keys[nkeys][32] in first-seen order — the
 * numbering of cv_diag_dedupe_keys — d_key_index[n] (uint32) and *d_nkeys (one uint32), what
 * cv_ed25519_verify_device_keyed takes for a batch whose keys are already resident.  Two keys are equal iff their 32
 * bytes are; nothing is decoded.  The result depends on the input bytes alone.  d_keys holds n * 32 bytes (rows from
 * nkeys on are not written), d_key_index n * 4, d_workspace cv_ed25519_dedupe_keys_workspace(n) bytes (overwritten;
 * nothing is expected in it); d_nkeys is 4-byte aligned, the others as under the alignment rules above.  Enqueues on
 * `stream` and returns without synchronising; n == 0 enqueues nothing; n > 0xfffffffe: CV_E_TOO_LARGE.  A probe of
 * the call's hash table that found no slot — the table's size rules it out — leaves *d_nkeys = 0xffffffff.
 * cv_ed25519_dedupe_keys_workspace runs on the host and needs no device (0 for n > 0xfffffffe). */
int cv_ed25519_dedupe_keys_device(cv_ctx *ctx, int device, size_t n, const void *d_pk, void *d_keys, void *d_key_index,
                                  void *d_nkeys, void *d_workspace, void *stream);
uint64_t cv_ed25519_dedupe_keys_workspace(size_t n);

/* The hot-key route: N x PublicKey.verifyWithECDSA (CryptoUtilities.kt:90-96) for a batch whose keys
 * are skewed — a few keys that sign thousands of records beside a long tail of keys seen once.  The batch is split on
 * the device by how often each key occurs: the records of hot keys go through the keyed comb, the rest through the
 * unkeyed path, and d_bitmap / d_status (optional) are, record for record, those of cv_ed25519_verify_device; inputs,
 * alignment and outputs are that call's.  With the keys numbered in first-seen order (cv_ed25519_dedupe_keys_device), a
 * key is a candidate iff it occurs at least hot_min times, and hot iff it is among the first cv_key_cache_reserve
 * candidates in first-seen order (the pool never grows for this call; later candidates are cold).  hot_min 0 means 8;
 * 1 makes every key hot up to the capacity; a value above n makes every record cold.  The classes depend on the input
 * bytes alone.  d_workspace: cv_ed25519_verify_hotkeys_workspace(n) bytes, 16-byte aligned (overwritten; nothing is
 * expected in it; it must stay untouched until the work on `stream` has finished).  route_out (host, optional) =
 * {distinct keys, hot keys, hot records, cold records}.  The call synchronises `stream` ONCE, to read the hot key rows
 * back (32 B each, resolved against the key pool as cv_ed25519_verify_device_keyed resolves its keys; cv_key_cache_stats
 * counts one lookup per hot key row), then enqueues the rest and returns without synchronising again.  As for the
 * keyed call, keyed calls on one device must share one stream.  n == 0 returns CV_OK and touches nothing;
 * n > 0xfffffffe: CV_E_TOO_LARGE; a NULL ctx or required pointer: CV_E_ARGS — all before any device work.
 * cv_ed25519_verify_hotkeys_workspace runs on the host and needs no device (0 for n > 0xfffffffe). */
int cv_ed25519_verify_device_hotkeys(cv_ctx *ctx, int device, size_t n, const void *d_pk, const void *d_sig,
                                     const void *d_arena, const void *d_off, const void *d_len, void *d_bitmap,
                                     void *d_status /* optional */, uint32_t hot_min, void *d_workspace,
                                     void *stream, uint32_t route_out[4] /* host, optional */);
uint64_t cv_ed25519_verify_hotkeys_workspace(size_t n);

int cv_ed25519_sign_device(cv_ctx *ctx, int device, size_t n, const void *d_seed, const void *d_arena,
                           const void *d_off, const void *d_len, void *d_pk, void *d_sig, void *stream);

/* Device-resident form of cv_ed25519_sign_keyed (KeyPair.signWithECDSA, CryptoUtilities.kt:63-73; NotaryFlow.kt:97-113):
 * d_sig[n][64] from the signer's record on `device`; enqueued on `stream` (NULL: the device's own) without
 * synchronising, like cv_ed25519_verify_device, so a verify of the signatures queued behind it on the same stream
 * reads them complete.  The signer stays open until that work has finished. */
int cv_ed25519_sign_keyed_device(cv_ctx *ctx, int device, const cv_signer *s, size_t n, const void *d_arena,
                                 const void *d_off, const void *d_len, void *d_sig, void *stream);

/* d_workspace: nleaves * 32 bytes (leaf digests, overwritten) */
int cv_merkle_tx_ids_device(cv_ctx *ctx, int device, size_t ntx, size_t nleaves, const void *d_arena,
                            const void *d_leaf_off, const void *d_leaf_len, const void *d_tx_leaf_begin,
                            void *d_workspace, void *d_ids, void *d_tx_status, void *stream);

/* Device-resident form of cv_missing_signers (SignedTransaction.kt:58-72,89-93; CompositeKey.kt:49,75-81): the same
 * arrays as device pointers, d_workspace of cv_missing_signers_workspace(ntx, nnodes) bytes (overwritten; nothing is
 * expected in it).  Enqueues on `stream` and returns without synchronising or reading anything back, so it chains
 * behind cv_ed25519_verify_device on the same stream and takes that call's d_bitmap as it stands.  It TRUSTS
 * d_tx_req_begin, d_tx_sig_begin and d_req_begin (begin[0] == 0, monotone, the last entry equal to the count), as the
 * other device-resident calls trust their ranges; everything per node, d_child_begin included, is checked on the device
 * as in the host form.  d_req_allowed and d_bitmap may be NULL (none allowed; all valid). */
int cv_missing_signers_device(cv_ctx *ctx, int device, size_t ntx, size_t nreq, size_t nnodes, size_t nchild, size_t nsig,
                              const void *d_kind, const void *d_leaf_key, const void *d_threshold,
                              const void *d_child_begin, const void *d_child, const void *d_weight,
                              const void *d_req_begin, const void *d_tx_req_begin, const void *d_sig_key,
                              const void *d_tx_sig_begin, const void *d_req_allowed, const void *d_bitmap,
                              uint32_t wide_min, void *d_req_missing, void *d_tx_status, void *d_workspace, void *stream);

/* Block until all work the context enqueued on `device` has finished. */
int cv_synchronize(cv_ctx *ctx, int device);

/* ---------------------------------------------------------------- roofline calibration
 * Measures, on `device`, the chip-wide issue rate of the 32x32->64 multiply-accumulate
 * (v_mad_u64_u32) the field arithmetic is built on, and the practical GF(2^255-19) multiply rate of
 * the engine's fe_mul.  Either output pointer may be NULL.  Used by bench.py for roofline.peak.
 */
int cv_calibrate(cv_ctx *ctx, int device, double *mad_per_s, double *femul_per_s);

/* The same multiply-accumulate peak on a cycle basis: out[5] = {MAC/s, shader clock in GHz read
 * in-kernel (s_memtime over s_memrealtime), cycles per v_mad_u64_u32 wave-instruction per SIMD,
 * SIMD count, MAC/s ceiling at the 2.4 GHz peak clock for that cycle count}. */
int cv_calibrate_cycles(cv_ctx *ctx, int device, double *out);

/* ---------------------------------------------------------------- options
 * Per-context tuning, read at the start of every call (cv_set_option from any thread; a call in progress
 * keeps the values it started with).  Defaults are the measured best on MI355X; the kernel-form
 * thresholds also let tests force each form on any batch size.  CV_E_ARGS for an unknown option or a value
 * out of range. */
#define CV_OPT_TRI_MAX 1            /* batches up to this many signatures: tri-chain latency kernels (4096; 0 = never) */
#define CV_OPT_QUAD_MAX 2           /* up to this: quad latency kernels (32768; 0 = never); above: throughput kernels */
#define CV_OPT_DRAIN_SPLIT 3        /* throughput chunks' drain overlap: 0 off, 1 auto (default), 2 always */
#define CV_OPT_DRAIN_SPLIT_PCT 4    /* the overlapped tail's share of a split chunk, percent (10) */
#define CV_OPT_PIPE_MIN 5           /* host batches (per device) above this are pipelined (131072) */
#define CV_OPT_PIPE_FIRST 6         /* first sub-chunk of a synchronous pipelined call (32768; sizes then double) */
#define CV_OPT_PIPE_CHUNK 7         /* largest sub-chunk of a synchronous pipelined call (262144); a call of n records
                                       uses about n / 16 per sub-chunk, at least 2 x CV_OPT_PIPE_FIRST */
#define CV_OPT_ASYNC_CHUNK 8        /* sub-chunk unit of the asynchronous calls: 1 or 2 of them per launch group, the
                                       multiple nearest n / 16 (196608 = one round of resident verify waves) */
#define CV_OPT_HOST_THREADS 9       /* host threads per device packing pageable inputs / deduping keys (8) */
#define CV_OPT_SMALL_ZERO_COPY 10   /* tri-form host batches: 0 DMA, 1 zero-copy reads, 2 gather kernel, 3 auto (default) */
#define CV_OPT_SMALL_DIRECT_MIN 11  /* unpipelined batches from pinned inputs DMA them in place from this size (16384) */
#define CV_OPT_AUTO_KEYED 12        /* host dedupe + keyed path for repeated keys: 1 on (default), 0 off */
#define CV_OPT_SHARD_MIN 13         /* routing: batches up to this go whole to one device; fewer per shard never (4096) */
#define CV_OPT_SPREAD_MIN 14        /* routing: batches from this size are cut over all devices (262144) */
#define CV_OPT_MERKLE_CHUNK 15      /* leaves per Merkle pipeline sub-chunk (262144) */
#define CV_OPT_PREP_OVERLAP_MIN 16  /* unpipelined host batches from this size send keys and signatures first and
                                       decode their points on a helper stream while the rest of their inputs is still
                                       in DMA (32768) */
#define CV_OPT_TIMELINE 17          /* diagnostics: 1 = time each synchronous pipelined call on the GPU (HIP events per
                                       sub-chunk, read back as CV_STATS_TIMELINE); 0 off (default) */
#define CV_OPT_PIPE_SPLIT 18        /* synchronous pipelined calls: about n / this records per sub-chunk after the ramp,
                                       clamped to [2 x CV_OPT_PIPE_FIRST, CV_OPT_PIPE_CHUNK] (16) */
#define CV_OPT_PIPE_OVERLAP_FIRST 19 /* synchronous pipelined calls: the first sub-chunk's keys and signatures go first and
                                       its point decodes start as soon as they land: 1 on, 0 off (default: measured
                                       neutral — the ramp shortens, the call does not) */
#define CV_OPT_MID_PIECES 20        /* unpipelined mid-size batches from pageable inputs: packed and DMAed in up to this
                                       many pieces (about 1 MB of keys + signatures each), the DMA of one piece beside
                                       the packing of the next (1 = one DMA per part, the default: measured neutral to
                                       slower at 65,536) */
#define CV_OPT_PIPE_SLOTS 21        /* compute streams (workspace slots) a pipelined verify call deals its sub-chunks over
                                       (2; 3 or 4 allowed) */
#define CV_OPT_TXS_MERKLE_STREAM 22 /* cv_verify_transactions: the stream its Merkle groups run on — 0 the compute streams
                                       beside the signature groups, 1 the copy stream behind their leaves, 2 a stream
                                       of their own (default) */
#define CV_OPT_FUSED_KEYED 23       /* cv_notarise_batch (validating) and cv_resolve_batch: the keyed verify path over the
                                       keys the device dedupe finds — 0 never, 1 auto (more than CV_OPT_TRI_MAX signatures,
                                       at least eight per distinct key, no more distinct keys than the key pool's
                                       capacity), 2 whenever the distinct keys fit the pool's capacity; 3 the hot-key
                                       route (keys that occur at least 8 times keyed, the rest unkeyed)
                                       for more than CV_OPT_TRI_MAX signatures, 4 the hot-key route for any batch with
                                       keys that occur at least twice hot (tests at small shapes).  Every output is
                                       the same under all five.  Default 0: auto cost a resolve chain more than its keyed
                                       verify saved */
#define CV_OPT_COUNT 24
int cv_set_option(cv_ctx *ctx, int option, int64_t value);
int cv_get_option(cv_ctx *ctx, int option, int64_t *value);

/* Diagnostics (no reference counterpart): the context's counters since the last reset; returns the number
 * of values of that kind (fills at most nout of them), or CV_E_ARGS.
 *   CV_STATS_PIPE  {plan, pack, wait, enqueue, sync seconds of the pipelined host path; calls; sub-chunks;
 *                   sub-chunks DMAed in place from pinned inputs}
 *   CV_STATS_SMALL {setup, pack (+ input DMA issue), launch, sync, assemble seconds of the unpipelined host path
 *                   (notary-sized batches: zero-copy and one-DMA forms); calls}
 *   CV_STATS_ROUTE {calls, routed whole to one device, cut over several, shards, keyed shards, keyed
 *                   sub-chunks, Merkle calls, Merkle sub-chunks}
 *   CV_STATS_TIMELINE {sums over the synchronous pipelined calls (cv_ed25519_verify_batch, cv_verify_transactions)
 *                   timed with CV_OPT_TIMELINE = 1, in ms from each call's first input DMA: first kernel start (the
 *                   ramp), last input DMA end, last kernel end (the span), kernel-busy time (union over the launch
 *                   groups), idle gaps between the first kernel start and the span's end, the tail after the last DMA,
 *                   the result copy (host-timed); first sub-chunk records; Merkle-group busy, verify-group busy, last
 *                   Merkle DMA end (ms; cv_verify_transactions); launch groups; host time from the call's entry to
 *                   its first input DMA enqueued (verify calls) and from the GPU work joined to the results in the
 *                   caller's arrays (ms); calls timed}
 *   CV_STATS_RESOLVE {sums over the cv_resolve_batch calls timed with CV_OPT_TIMELINE = 1, in ms: upload, leaf hashes
 *                   and trees, join (table clear, insert, probe), signature verify, missing signers, gate, read-back
 *                   (HIP events around the stages), host order and walk (host-timed); calls timed} */
#define CV_STATS_PIPE 0
#define CV_STATS_SMALL 1
#define CV_STATS_ROUTE 2
#define CV_STATS_TIMELINE 3
#define CV_STATS_RESOLVE 4
int cv_diag_stats(cv_ctx *ctx, int which, double *out, size_t nout, int reset);

/* max(msg_off[i] + msg_len[i]) over n records (0 for n = 0): the arena bytes a batch reaches, for the
 * shim's bounds check before a call (multi-threaded above 2^20 records).  Host only. */
uint64_t cv_msg_extent(size_t n, const uint64_t *msg_off, const uint32_t *msg_len);

/* Diagnostics: the host-side key dedupe cv_ed25519_verify_batch runs before choosing the keyed path
 * (seeded hash of all 32 key bytes).  Returns 1 and fills key_index[n] / *nkeys (distinct keys in
 * first-seen order) when the batch repeats keys enough for the keyed path (n >= 64, at least eight
 * signatures per distinct key), else 0.  Above 4,096 signatures a sample of 4 sqrt(n) (512 .. 4,096) at
 * pseudo-random positions first estimates the repetition (birthday count) and a batch estimated below four
 * signatures per key is taken as distinct-keyed without hashing the rest.  Host only: needs no device and no
 * context. */
int cv_diag_dedupe_keys(size_t n, const uint8_t *pk, uint32_t *key_index, size_t *nkeys);

#ifdef __cplusplus
}
#endif
#endif /* CORDAVERIFY_H */
