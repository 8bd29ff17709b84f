// cv_resolve.h — the graph half of cv_resolve_batch: the body of ResolveTransactionsFlow.call (core/src/main/kotlin/
// net/corda/flows/ResolveTransactionsFlow.kt:96-128) over the transactions downloadDependencies returned, in download
// order (resultQ.values).  The per-lane core of cv_k_resolve.hip is __host__ __device__, so tests/resolve_harness.cpp
// runs the lanes on the CPU one after another, in any order (the atomics reduce to plain operations there); the order
// and the walk are plain host C++ below, the same code in the library, the harness and the sanitizer program.
//
// THREE KERNELS, no lane reading what another lane of its kernel writes except through an atomic:
//   insert  per transaction t: atomicCAS(slot, NONE, t) into a batch-local table of transaction INDICES over the
//           CLAIMED ids (stx.id is what resultQ and forwardGraph are keyed by, :39-45,:170): a table of cv_table.h
//           (probing, sizing and hashing are described there; a floor of 2 slots).  A loser compares
//           its id with the occupant's — both in the immutable input — and probes on, or, on equality, does
//           atomicMin(slot, t) and atomicMin(dstat[DUP], min(t, occupant)): the slot ends at the smallest index that
//           carries the id and DUP at the smallest index whose id occurs more than once, whichever lane won.
//   probe   per input i, the table read-only by then (the kernel boundary publishes it): input_dep[i] = the
//           transaction whose claimed id equals input_txhash[i] or NONE (`forwardGraph.getOrPut(input.txhash)`, :43;
//           NONE: a transaction the node already stores, by construction of downloadDependencies, :158-174);
//           input_status[i] = 0 external, 1 in the batch and input_index < tx_output_count[dep], 2 in the batch and
//           out of range (`it.tx.outputs[stateRef.index]`, ServiceHub.kt:46-49).
//   gate    per transaction: outcome[t], first match wins in the order stx.toLedgerTransaction meets them (:107;
//           SignedTransaction.kt:134 -> verifySignatures() without keys, then the inputs resolved one by one) —
//             EMPTY, ID_MISMATCH       the `tx` getter (SignedTransaction.kt:34-38)
//             TX_INVALID, BAD_KEY      checkSignaturesAreValid (:82-87): the FIRST failing signature settles the
//                                      class, by the rules of cvn_gate; no signatures at all is TX_INVALID
//             MALFORMED, SIGNATURES_MISSING   the missing-signers status (cv_ck.h), no key allowed to be missing
//             BAD_INPUT                some input's status is 2; bad_input[t] = the first such input
//           atomicMin(dstat[BADID], t) for EMPTY / ID_MISMATCH; the external inputs are added to dstat[EXTERNAL].
// NO LANE WAITS FOR ANOTHER LANE: no spin, lock or flag.  EVERY PROBE IS BOUNDED: each is cv_walk (cv_table.h), which
// looks at no more than the slot count, and sets dstat[CVR_D_ERROR] when it runs out (the host returns CV_E_HIP).
//
// HOST, after the one read-back (a lexicographic depth-first order is inherently sequential):
//   cvr_order  topologicalSort (:37-67): the dependents of every transaction — distinct, in ascending index order,
//              what the LinkedHashSet of :43 holds when the transactions are iterated in order — then visit() in
//              input order with the visited set, post-order, reversed.  An explicit stack: the reference recurses, a
//              chain of 2^20 transactions must not overflow ours.
//   cvr_walk   the loop of :105-111: the leading transactions of `order` that pass everything checked here, and what
//              stops it — a transaction's outcome, or, going through its inputs in order, a dependency in the batch
//              that does not stand earlier in `order` (loadState finds nothing recorded: TransactionResolutionException;
//              only a self-reference or a cycle of hand-fed input_txhash gets there) before an out-of-range index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cv_notary.h"
#include "cv_uniq.h"

// outcome[t] (include/cordaverify.h CV_RS_*); 0-7 as CVN_*
#define CVR_OK 0
#define CVR_EMPTY 1
#define CVR_ID_MISMATCH 2
#define CVR_TX_INVALID 4
#define CVR_BAD_KEY 5
#define CVR_SIGNATURES_MISSING 6
#define CVR_MALFORMED 7
#define CVR_BAD_INPUT 9
#define CVR_UNRESOLVED 10          // STOP_CLASS only
#define CVR_NONE 0xffffffffu
// input_status[i]
#define CVR_IN_EXTERNAL 0
#define CVR_IN_OK 1
#define CVR_IN_RANGE 2
// graph[] (include/cordaverify.h CV_RG_*)
#define CVR_G_STATUS 0
#define CVR_G_WHICH 1
#define CVR_G_N_PASS 2
#define CVR_G_STOP_CLASS 3
#define CVR_G_STOP_TX 4
#define CVR_G_STOP_INPUT 5
#define CVR_G_EXTERNAL 6
#define CVR_G_MAXPROBE 7
#define CVR_G_WRAPS 8
#define CVR_G_WORDS 9
#define CVR_GS_OK 0
#define CVR_GS_BAD_ID 1
#define CVR_GS_DUPLICATE_ID 2
// words of the call's device counters: the first four start at 0xffffffff (an atomicMin's identity), the rest at 0
#define CVR_D_DUP 0                // smallest index of a transaction whose id occurs more than once
#define CVR_D_BADID 1              // smallest index of a transaction that is EMPTY or ID_MISMATCH
#define CVR_D_ERROR 4              // a probe loop ran out of slots
#define CVR_D_MAXPROBE 5           // longest probe (slots looked at)
#define CVR_D_WRAPS 6              // probes that passed the last slot
#define CVR_D_EXTERNAL 7           // inputs of status 0
#define CVR_D_WORDS 8

struct CvResolve {
    uint32_t ntx, ninputs;
    const uint32_t *claimed;           // ntx * 8: the words of the claimed id bytes
    uint32_t *tab, mask;               // mask + 1 slots, CVR_NONE = empty
    uint64_t seed;
    const uint32_t *tx_input_begin;    // ntx + 1
    const uint32_t *input_txhash;      // ninputs * 8
    const uint32_t *input_index;       // ninputs
    const uint32_t *tx_output_count;   // ntx
    uint32_t *input_dep;               // ninputs
    uint8_t *input_status;             // ninputs
    // gate
    const uint8_t *mstatus;            // ntx: the Merkle status (non-zero = no leaves)
    const uint32_t *id;                // ntx * 8: the recomputed ids
    const uint32_t *tx_sig_begin;      // ntx + 1
    const uint64_t *bitmap;            // the verify's verdict bits
    const uint8_t *sig_status;         // nsig: CV_SIG_*
    const uint8_t *sig_pre;            // nsig, or null = none
    const uint8_t *ck_status;          // ntx: CV_VS_*
    uint8_t *outcome;                  // ntx
    uint32_t *first_bad, *bad_input;   // ntx each
    uint32_t *dstat;                   // CVR_D_WORDS
};

CV_HD void cvr_insert(const CvResolve &R, uint32_t t) {
    const uint32_t *k = R.claimed + 8 * (size_t)t;
    // the CAS first; on an equal id atomicMin on the slot unconditionally and on CVR_D_DUP; wraps and max-probe counted
    uint32_t *const wraps = R.dstat + CVR_D_WRAPS;
    const CvWalk<uint32_t> w = cv_walk(R.mask, (uint32_t)cvu_hash(k, R.seed), wraps, [&](uint32_t slot) {
        const uint32_t old = cvu_atomic_cas(R.tab + slot, CVR_NONE, t);
        if (old == CVR_NONE) return true;
        // `old` may already have been lowered by another loser of the same id: any holder of the slot carries that id
        if (!cvu_key_eq(R.claimed + 8 * (size_t)old, k)) return false;
        cvu_atomic_min(R.tab + slot, t);
        cvu_atomic_min(R.dstat + CVR_D_DUP, t < old ? t : old);
        return true;
    });
    if (!w.stopped) R.dstat[CVR_D_ERROR] = 1;   // more transactions than slots: the caller sized the table at twice
    cvu_note_max(R.dstat + CVR_D_MAXPROBE, w.n);
}

CV_HD void cvr_probe(const CvResolve &R, uint32_t i) {
    const uint32_t *k = R.input_txhash + 8 * (size_t)i;
    uint32_t dep = CVR_NONE;
    // read-only, the o < R.ntx guard kept; wraps and max-probe counted
    uint32_t *const wraps = R.dstat + CVR_D_WRAPS;
    const CvWalk<uint32_t> w = cv_walk(R.mask, (uint32_t)cvu_hash(k, R.seed), wraps, [&](uint32_t slot) {
        const uint32_t o = R.tab[slot];
        if (o == CVR_NONE) return true;
        if (o >= R.ntx || !cvu_key_eq(R.claimed + 8 * (size_t)o, k)) return false;
        dep = o;
        return true;
    });
    if (!w.stopped) R.dstat[CVR_D_ERROR] = 1;   // a full table without the id: the slot count rules it out
    cvu_note_max(R.dstat + CVR_D_MAXPROBE, w.n);
    R.input_dep[i] = dep;
    R.input_status[i] = dep == CVR_NONE ? CVR_IN_EXTERNAL : R.input_index[i] < R.tx_output_count[dep] ? CVR_IN_OK : CVR_IN_RANGE;
}

CV_HD void cvr_gate(const CvResolve &R, uint32_t t) {
    uint32_t out = CVR_OK, bad = CVN_NO_SIG, bin = CVR_NONE, ext = 0;
    const uint32_t ib = R.tx_input_begin[t], ie = R.tx_input_begin[t + 1];
    for (uint32_t i = ib; i < ie; i++) {
        const uint32_t st = R.input_status[i];
        ext += st == CVR_IN_EXTERNAL;
        if (st == CVR_IN_RANGE && bin == CVR_NONE) bin = i;
    }
    if (R.mstatus[t])
        out = CVR_EMPTY;
    else {
        uint32_t diff = 0;
        for (int q = 0; q < 8; q++) diff |= R.id[(size_t)t * 8 + q] ^ R.claimed[(size_t)t * 8 + q];
        if (diff)
            out = CVR_ID_MISMATCH;
        else {
            CvNotary N{};
            N.bitmap = R.bitmap, N.sig_pre = R.sig_pre;
            const uint32_t b = R.tx_sig_begin[t], e = R.tx_sig_begin[t + 1];
            bad = cvn_first_bad(N, b, e);
            if (bad != CVN_NO_SIG) {
                const uint32_t p = R.sig_pre ? R.sig_pre[bad] : 0;
                out = p == CVN_PRE_KEY || (p == 0 && R.sig_status[bad] == CVN_SIG_BAD_KEY) ? CVR_BAD_KEY : CVR_TX_INVALID;
            } else if (e == b)
                out = CVR_TX_INVALID;
            else if (R.ck_status[t] == CVN_VS_MALFORMED)
                out = CVR_MALFORMED;
            else if (R.ck_status[t] == CVN_VS_MISSING)
                out = CVR_SIGNATURES_MISSING;
            else if (bin != CVR_NONE)
                out = CVR_BAD_INPUT;
        }
    }
    if (out == CVR_EMPTY || out == CVR_ID_MISMATCH) cvu_atomic_min(R.dstat + CVR_D_BADID, t);
    if (ext) cvu_atomic_add(R.dstat + CVR_D_EXTERNAL, ext);
    R.outcome[t] = (uint8_t)out;
    R.first_bad[t] = bad;
    R.bad_input[t] = out == CVR_BAD_INPUT ? bin : CVR_NONE;
}

// ---------------------------------------------------------------- host: the table's size, the order, the walk
#ifndef __HIP_DEVICE_COMPILE__
#include <algorithm>
#include <vector>

// slots of the join table: a power of two, at least 2 ntx (ntx <= 2^30)
inline uint32_t cvr_slots(size_t ntx) { return (uint32_t)cv_table_slots(ntx, 2); }

// topologicalSort over input_dep; order gets ntx entries.  No two transactions share an id (the caller checked).
inline void cvr_order(uint32_t ntx, const uint32_t *tx_input_begin, const uint32_t *input_dep, uint32_t *order) {
    // the dependents of d: begin[d] .. begin[d + 1] of list, distinct (t ascends, so a repeat is the last one added)
    std::vector<uint32_t> begin((size_t)ntx + 1, 0), last(ntx, CVR_NONE);
    for (uint32_t t = 0; t < ntx; t++)
        for (uint32_t i = tx_input_begin[t]; i < tx_input_begin[t + 1]; i++) {
            const uint32_t d = input_dep[i];
            if (d >= ntx || last[d] == t) continue;
            last[d] = t;
            begin[(size_t)d + 1]++;
        }
    for (uint32_t d = 0; d < ntx; d++) begin[(size_t)d + 1] += begin[d];
    std::vector<uint32_t> list(begin[ntx]), cur(begin.begin(), begin.end() - 1);
    std::fill(last.begin(), last.end(), CVR_NONE);
    for (uint32_t t = 0; t < ntx; t++)
        for (uint32_t i = tx_input_begin[t]; i < tx_input_begin[t + 1]; i++) {
            const uint32_t d = input_dep[i];
            if (d >= ntx || last[d] == t) continue;
            last[d] = t;
            list[cur[d]++] = t;
        }
    // visit(): cur[v] walks v's dependents; a transaction is emitted when they are exhausted (post-order), and the
    // result is reversed by filling order from its end
    std::vector<uint8_t> visited(ntx, 0);
    std::vector<uint32_t> stack;
    for (uint32_t d = 0; d < ntx; d++) cur[d] = begin[d];
    uint32_t pos = ntx;
    for (uint32_t r = 0; r < ntx; r++) {
        if (visited[r]) continue;
        visited[r] = 1;
        stack.push_back(r);
        while (!stack.empty()) {
            const uint32_t v = stack.back();
            if (cur[v] < begin[(size_t)v + 1]) {
                const uint32_t c = list[cur[v]++];
                if (!visited[c]) {
                    visited[c] = 1;
                    stack.push_back(c);
                }
            } else {
                order[--pos] = v;
                stack.pop_back();
            }
        }
    }
}

// the loop of :105-111 over order; fills graph[N_PASS .. STOP_INPUT]
inline void cvr_walk(uint32_t ntx, const uint32_t *tx_input_begin, const uint32_t *input_dep, const uint8_t *input_status,
                     const uint8_t *outcome, const uint32_t *bad_input, const uint32_t *order, uint32_t *graph) {
    std::vector<uint32_t> pos(ntx);
    for (uint32_t p = 0; p < ntx; p++) pos[order[p]] = p;
    graph[CVR_G_N_PASS] = ntx;
    graph[CVR_G_STOP_CLASS] = graph[CVR_G_STOP_TX] = graph[CVR_G_STOP_INPUT] = CVR_NONE;
    for (uint32_t p = 0; p < ntx; p++) {
        const uint32_t t = order[p];
        uint32_t cls = CVR_OK, in = CVR_NONE;
        if (outcome[t] != CVR_OK && outcome[t] != CVR_BAD_INPUT)
            cls = outcome[t], in = bad_input[t];
        else
            for (uint32_t i = tx_input_begin[t]; i < tx_input_begin[t + 1] && cls == CVR_OK; i++) {
                const uint32_t d = input_dep[i];
                if (d >= ntx) continue;
                if (pos[d] >= p)
                    cls = CVR_UNRESOLVED, in = i;
                else if (input_status[i] == CVR_IN_RANGE)
                    cls = CVR_BAD_INPUT, in = i;
            }
        if (cls != CVR_OK) {
            graph[CVR_G_N_PASS] = p;
            graph[CVR_G_STOP_CLASS] = cls, graph[CVR_G_STOP_TX] = t, graph[CVR_G_STOP_INPUT] = in;
            return;
        }
    }
}

// Everything after the read-back: graph[] and order[] from the per-lane outputs and the device counters.  BAD_ID takes
// precedence over DUPLICATE_ID: the reference's download rounds, which are not an input here, could interleave the
// `tx` getter of :167 with the check of :170 either way, and both fail the flow.  Returns false on a probe error.
inline bool cvr_finish(uint32_t ntx, const uint32_t *tx_input_begin, const uint32_t *input_dep, const uint8_t *input_status,
                       const uint8_t *outcome, const uint32_t *bad_input, const uint32_t *dstat, uint32_t *order,
                       uint32_t *graph) {
    if (dstat[CVR_D_ERROR]) return false;
    graph[CVR_G_EXTERNAL] = dstat[CVR_D_EXTERNAL];
    graph[CVR_G_MAXPROBE] = dstat[CVR_D_MAXPROBE];
    graph[CVR_G_WRAPS] = dstat[CVR_D_WRAPS];
    const bool badid = dstat[CVR_D_BADID] != CVR_NONE, dup = dstat[CVR_D_DUP] != CVR_NONE;
    graph[CVR_G_STATUS] = badid ? CVR_GS_BAD_ID : dup ? CVR_GS_DUPLICATE_ID : CVR_GS_OK;
    graph[CVR_G_WHICH] = badid ? dstat[CVR_D_BADID] : dstat[CVR_D_DUP];
    if (badid || dup) {
        for (uint32_t t = 0; t < ntx; t++) order[t] = 0;
        graph[CVR_G_N_PASS] = 0;
        graph[CVR_G_STOP_CLASS] = graph[CVR_G_STOP_TX] = graph[CVR_G_STOP_INPUT] = CVR_NONE;
        return true;
    }
    cvr_order(ntx, tx_input_begin, input_dep, order);
    cvr_walk(ntx, tx_input_begin, input_dep, input_status, outcome, bad_input, order, graph);
    return true;
}
#endif
