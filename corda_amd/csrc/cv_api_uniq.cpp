// cv_api_uniq.cpp — the device-resident uniqueness set of the C-ABI (include/cordaverify.h): the cv_uniq_* entry
// points and the decision helpers cv_api_notary.cpp shares (cvh::uniq_*).  The engine state, struct cv_uniq included,
// is cv_host.h's; the range check and the workspace's layout are cv_batch.h's.
#include "cv_batch.h"

using namespace cvh;

// ---------------------------------------------------------------- uniqueness set (the notary's commit step)

#define CV_UNIQ_SNAP_BLOCK 256u   // slots per block of the snapshot's kernels (cv_k_uniq.hip: CV_BLOCK)

namespace cvh {
// the frame's stat_end, and the set's extra: its wraps
int uniq_stat_end(cv_uniq *u) {
    const int rc = u->stat_end();
    u->wraps += u->hstat[CVU_D_WRAPS];
    return rc;
}

// The decision of one batch on the set's stream: front, then rounds while the device says a request is undecided (one
// 4-byte read-back per round), then the serial tail for what max_rounds left (with no round run the count is unknown
// and the tail looks for itself), report + insert.  Shared by cv_uniq_commit_batch and cv_notarise_batch.
int uniq_decide(cv_uniq *u, const CvUniqBatch &B, uint32_t *cur, uint32_t *nxt, uint64_t *rounds_out) {
    hipStream_t s = u->stream;
    u->touch();                                                  // a commit may insert: passes of a snapshot end here
    CV_TRY(cvk_uniq_front(&u->T, &B, cur, s));
    uint64_t rounds = 0;
    bool undecided = true;
    while (undecided && rounds < (uint64_t)u->max_rounds) {
        CV_TRY(cvk_uniq_round(&B, cur, nxt, (uint32_t)rounds, s));
        std::swap(cur, nxt);
        CV_TRY(hipMemcpyAsync(u->hstat, B.dstat + CVU_D_ROUND0 + rounds, 4, hipMemcpyDeviceToHost, s));
        CV_TRY(hipStreamSynchronize(s));
        undecided = u->hstat[0] != 0;
        rounds++;
    }
    CV_TRY(cvk_uniq_finish(&u->T, &B, cur, undecided ? 1 : 0, s));
    *rounds_out = rounds;
    return CV_OK;
}
}  // namespace cvh

extern "C" {

int cv_uniq_open(cv_ctx *ctx, int device, size_t capacity_states, cv_uniq **out) {
    int rc = Resident::open_check(ctx, device, capacity_states, out);
    if (rc != CV_OK) return rc;
    std::unique_ptr<cv_uniq> u(new (std::nothrow) cv_uniq());
    if (!u) return CV_E_OOM;
    std::random_device rd;
    const uint64_t seed = key_seed(0) ^ rand64(rd);
    u->epoch = rand64(rd) | 1;                                   // a cursor of another set does not continue on this one
    rc = u->open(ctx, device, capacity_states, CVU_SLOT_BYTES, CVU_D_WORDS, false);   // freed, not overwritten
    if (rc != CV_OK) {
        cv_uniq_close(u.release());
        return rc;
    }
    u->T = cvu_carve(u->tab, u->slots, seed);
    *out = u.release();
    return CV_OK;
}

void cv_uniq_close(cv_uniq *u) {
    if (!u) return;
    u->close([u] {
        u->nws.release();
        u->nin.release();
        u->nout.release();
    });
    delete u;
}

int cv_uniq_reserve(cv_uniq *u, size_t capacity_states) {
    if (!u) return CV_E_ARGS;
    if (capacity_states > kUniqMaxStates) return CV_E_TOO_LARGE;
    std::lock_guard<std::mutex> g(u->mu);
    CvUniqTable to{};
    bool rehashed = false;
    const int rc = u->grow(
        capacity_states,
        [&](void *base, size_t slots) {
            to = cvu_carve(base, slots, u->T.seed);
            return cvk_uniq_rehash(&u->T, &to, u->dstat.as<uint32_t>(), u->stream);
        },
        [u] { return uniq_stat_end(u); }, &rehashed);
    if (rehashed) {
        u->T = to;
        u->touch();                                              // the slots moved
    }
    return rc;
}

int cv_uniq_set_max_rounds(cv_uniq *u, int rounds) {
    if (!u || rounds < 0 || rounds > CVU_MAX_ROUNDS) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(u->mu);
    u->max_rounds = rounds;
    return CV_OK;
}

int cv_uniq_stats(cv_uniq *u, uint64_t *out, size_t nout) {
    if (!u || (nout && !out)) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(u->mu);
    const uint64_t v[CV_UNIQ_STAT_COUNT] = {u->resident, u->capacity, (uint64_t)u->slots, u->last_rounds,
                                            u->last_tail, u->last_probe, u->wraps};
    for (size_t k = 0; k < nout; k++) out[k] = k < CV_UNIQ_STAT_COUNT ? v[k] : 0;
    return CV_OK;
}

int cv_uniq_commit_batch(cv_uniq *u, size_t ntx, const uint8_t *state_key, const uint32_t *tx_state_begin,
                         const uint8_t *tx_id, const uint32_t *caller, const uint8_t *tx_enable, uint8_t *tx_status,
                         uint8_t *state_conflict, uint8_t *consumed_id, uint32_t *consumed_index,
                         uint32_t *consumed_caller) {
    if (ntx == 0) return CV_OK;
    if (ntx > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (!tx_state_begin || !tx_id || !caller || !tx_status) return CV_E_ARGS;
    if (!ranges_ok(tx_state_begin, ntx)) return CV_E_ARGS;
    const size_t S = tx_state_begin[ntx];
    if (S > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (S && (!state_key || !state_conflict || !consumed_id || !consumed_index || !consumed_caller)) return CV_E_ARGS;
    if (ntx > kUniqMaxStates || S > kUniqMaxStates) return CV_E_TOO_LARGE;
    if (!u) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(u->mu);
    if (u->resident + S > u->capacity) return CV_E_OOM;          // before any change and any output
    CV_TRY(hipSetDevice(u->ordinal));
    const size_t T = ntx, bs = uniq_bslots(S);
    // inputs | workspace | outputs (tx_status | state_conflict | consumed id, index, caller: one copy-back region)
    Layout lay;
    const size_t o_key = lay.take(32 * S), o_beg = lay.take(4 * (T + 1)), o_id = lay.take(32 * T), o_cal = lay.take(4 * T);
    const size_t o_en = lay.take(T), o_bt = lay.take(4 * bs), o_rep = lay.take(4 * S), o_res = lay.take(4 * S);
    const size_t o_stx = lay.take(4 * S), o_own = lay.take(4 * S), o_last = lay.take(4 * S), o_s0 = lay.take(4 * T);
    const size_t o_s1 = lay.take(4 * T), o_ts = lay.take(T), o_sc = lay.take(S), o_cid = lay.take(32 * S);
    const size_t o_cix = lay.take(4 * S), o_cc = lay.take(4 * S);
    CV_TRY(u->ws.ensure(lay.top + 16));
    uint8_t *base = u->ws.as<uint8_t>();
    hipStream_t s = u->stream;
    auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });   // the pageable copies read the caller's arrays
    if (S) CV_TRY(hipMemcpyAsync(base + o_key, state_key, 32 * S, hipMemcpyHostToDevice, s));
    CV_TRY(hipMemcpyAsync(base + o_beg, tx_state_begin, 4 * (T + 1), hipMemcpyHostToDevice, s));
    CV_TRY(hipMemcpyAsync(base + o_id, tx_id, 32 * T, hipMemcpyHostToDevice, s));
    CV_TRY(hipMemcpyAsync(base + o_cal, caller, 4 * T, hipMemcpyHostToDevice, s));
    if (tx_enable) CV_TRY(hipMemcpyAsync(base + o_en, tx_enable, T, hipMemcpyHostToDevice, s));
    CV_TRY(hipMemsetAsync(base + o_cid, 0, lay.top - o_cid, s));   // records of states without a conflict: zero
    int rc = u->stat_begin();
    if (rc != CV_OK) return rc;
    CvUniqBatch B{};
    B.ntx = (uint32_t)T;
    B.nstates = (uint32_t)S;
    B.key = at<uint32_t>(base, o_key);
    B.begin = at<uint32_t>(base, o_beg);
    B.id = at<uint32_t>(base, o_id);
    B.caller = at<uint32_t>(base, o_cal);
    B.enable = tx_enable ? base + o_en : nullptr;
    B.btab = at<uint32_t>(base, o_bt);
    B.bmask = (uint32_t)(bs - 1);
    B.rep = at<uint32_t>(base, o_rep);
    B.res = at<uint32_t>(base, o_res);
    B.state_tx = at<uint32_t>(base, o_stx);
    B.owner = at<uint32_t>(base, o_own);
    B.last = at<uint32_t>(base, o_last);
    B.tx_status = base + o_ts;
    B.state_conflict = base + o_sc;
    B.cons_id = at<uint32_t>(base, o_cid);
    B.cons_index = at<uint32_t>(base, o_cix);
    B.cons_caller = at<uint32_t>(base, o_cc);
    B.dstat = u->dstat.as<uint32_t>();
    uint64_t rounds = 0;
    rc = uniq_decide(u, B, at<uint32_t>(base, o_s0), at<uint32_t>(base, o_s1), &rounds);
    if (rc != CV_OK) return rc;
    CV_TRY(hipMemcpyAsync(tx_status, base + o_ts, T, hipMemcpyDeviceToHost, s));
    if (S) {
        CV_TRY(hipMemcpyAsync(state_conflict, base + o_sc, S, hipMemcpyDeviceToHost, s));
        CV_TRY(hipMemcpyAsync(consumed_id, base + o_cid, 32 * S, hipMemcpyDeviceToHost, s));
        CV_TRY(hipMemcpyAsync(consumed_index, base + o_cix, 4 * S, hipMemcpyDeviceToHost, s));
        CV_TRY(hipMemcpyAsync(consumed_caller, base + o_cc, 4 * S, hipMemcpyDeviceToHost, s));
    }
    rc = uniq_stat_end(u);
    drain.armed = false;
    u->resident += u->hstat[CVU_D_INSERTED];
    u->last_rounds = rounds;
    u->last_tail = u->hstat[CVU_D_TAIL];
    return rc;
}

int cv_uniq_lookup(cv_uniq *u, size_t n, const uint8_t *state_key, uint8_t *found, uint8_t *consumed_id,
                   uint32_t *consumed_index, uint32_t *consumed_caller) {
    if (n == 0) return CV_OK;
    if (n > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (!state_key || !found || !consumed_id || !consumed_index || !consumed_caller) return CV_E_ARGS;
    if (n > kUniqMaxStates) return CV_E_TOO_LARGE;
    if (!u) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(u->mu);
    CV_TRY(hipSetDevice(u->ordinal));
    Layout lay;
    const size_t o_key = lay.take(32 * n), o_f = lay.take(n), o_cid = lay.take(32 * n), o_cix = lay.take(4 * n);
    const size_t o_cc = lay.take(4 * n);
    CV_TRY(u->ws.ensure(lay.top + 16));
    uint8_t *base = u->ws.as<uint8_t>();
    hipStream_t s = u->stream;
    auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });
    CV_TRY(hipMemcpyAsync(base + o_key, state_key, 32 * n, hipMemcpyHostToDevice, s));
    CV_TRY(hipMemsetAsync(base + o_cid, 0, lay.top - o_cid, s));   // absent keys: zero records
    int rc = u->stat_begin();
    if (rc != CV_OK) return rc;
    CV_TRY(cvk_uniq_lookup(&u->T, (uint32_t)n, at<uint32_t>(base, o_key), base + o_f, at<uint32_t>(base, o_cid),
                           at<uint32_t>(base, o_cix), at<uint32_t>(base, o_cc), u->dstat.as<uint32_t>(), s));
    CV_TRY(hipMemcpyAsync(found, base + o_f, n, hipMemcpyDeviceToHost, s));
    CV_TRY(hipMemcpyAsync(consumed_id, base + o_cid, 32 * n, hipMemcpyDeviceToHost, s));
    CV_TRY(hipMemcpyAsync(consumed_index, base + o_cix, 4 * n, hipMemcpyDeviceToHost, s));
    CV_TRY(hipMemcpyAsync(consumed_caller, base + o_cc, 4 * n, hipMemcpyDeviceToHost, s));
    rc = uniq_stat_end(u);
    drain.armed = false;
    return rc;
}

// n rows into table T of the set's device (the set's own, or a fresh one beside it) on the set's stream: the check
// first (a key repeated in the call, or resident in T: CV_E_ARGS, T unchanged), then the inserts.  Synchronises.
static int uniq_load_into(cv_uniq *u, const CvUniqTable &T, size_t n, const uint8_t *state_key, const uint8_t *consumed_id,
                          const uint32_t *consumed_index, const uint32_t *consumed_caller) {
    const size_t bs = uniq_bslots(n);
    Layout lay;
    const size_t o_key = lay.take(32 * n), o_id = lay.take(32 * n), o_ix = lay.take(4 * n), o_cal = lay.take(4 * n);
    const size_t o_bt = lay.take(4 * bs), o_rep = lay.take(4 * n), o_res = lay.take(4 * n);
    CV_TRY(u->ws.ensure(lay.top + 16));
    uint8_t *base = u->ws.as<uint8_t>();
    hipStream_t s = u->stream;
    auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });
    CV_TRY(hipMemcpyAsync(base + o_key, state_key, 32 * n, hipMemcpyHostToDevice, s));
    CV_TRY(hipMemcpyAsync(base + o_id, consumed_id, 32 * n, hipMemcpyHostToDevice, s));
    CV_TRY(hipMemcpyAsync(base + o_ix, consumed_index, 4 * n, hipMemcpyHostToDevice, s));
    CV_TRY(hipMemcpyAsync(base + o_cal, consumed_caller, 4 * n, hipMemcpyHostToDevice, s));
    int rc = u->stat_begin();
    if (rc != CV_OK) return rc;
    CvUniqBatch B{};
    B.nstates = (uint32_t)n;
    B.key = at<uint32_t>(base, o_key);
    B.id = at<uint32_t>(base, o_id);
    B.cons_index = at<uint32_t>(base, o_ix);
    B.caller = at<uint32_t>(base, o_cal);
    B.btab = at<uint32_t>(base, o_bt);
    B.bmask = (uint32_t)(bs - 1);
    B.rep = at<uint32_t>(base, o_rep);
    B.res = at<uint32_t>(base, o_res);
    B.dstat = u->dstat.as<uint32_t>();
    // the check first (a key repeated in the call, or resident): the table changes only after it passed
    CV_TRY(cvk_uniq_load(&T, &B, 0, s));
    rc = u->stat_read();
    if (rc != CV_OK) return rc;
    if (u->hstat[CVU_D_ERROR]) {
        drain.armed = false;
        return CV_E_HIP;
    }
    if (u->hstat[CVU_D_BAD]) {
        drain.armed = false;
        return CV_E_ARGS;
    }
    CV_TRY(cvk_uniq_load(&T, &B, 1, s));
    rc = uniq_stat_end(u);
    drain.armed = false;
    return rc;
}

int cv_uniq_load(cv_uniq *u, size_t n, const uint8_t *state_key, const uint8_t *consumed_id,
                 const uint32_t *consumed_index, const uint32_t *consumed_caller) {
    if (n == 0) return CV_OK;
    if (n > 0xfffffffeull) return CV_E_TOO_LARGE;
    if (!state_key || !consumed_id || !consumed_index || !consumed_caller) return CV_E_ARGS;
    if (n > kUniqMaxStates) return CV_E_TOO_LARGE;
    if (!u) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(u->mu);
    if (u->resident + n > u->capacity) return CV_E_OOM;
    CV_TRY(hipSetDevice(u->ordinal));
    u->touch();
    const int rc = uniq_load_into(u, u->T, n, state_key, consumed_id, consumed_index, consumed_caller);
    if (rc == CV_OK) u->resident += n;
    return rc;
}

// The slot window of one snapshot call: what the load factor of 1/2 makes room for max_entries records, and no less
// than 65,536 slots, so a pass with a small buffer costs about resident / max_entries calls.
static uint64_t snap_window(uint64_t max_entries) { return std::max<uint64_t>(2 * max_entries, 65536); }

int cv_uniq_snapshot(cv_uniq *u, uint64_t cursor[2], size_t max_entries, uint8_t *state_key, uint8_t *consumed_id,
                     uint32_t *consumed_index, uint32_t *consumed_caller, size_t *n) {
    if (max_entries == 0 || !cursor || !n || !state_key || !consumed_id || !consumed_index || !consumed_caller)
        return CV_E_ARGS;
    if (max_entries > kUniqMaxStates) return CV_E_TOO_LARGE;
    if (!u) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(u->mu);
    if (cursor[0] == UINT64_MAX) {                               // a finished pass: nothing more
        *n = 0;
        return CV_OK;
    }
    const uint64_t slots = (uint64_t)u->T.mask + 1;
    if (cursor[0] == 0 ? cursor[1] != 0 : (cursor[1] != u->epoch || cursor[0] >= slots)) return CV_E_ARGS;
    CV_TRY(hipSetDevice(u->ordinal));
    const uint64_t b = cursor[0], e = std::min(slots, b + snap_window(max_entries));
    const size_t m = (size_t)std::min<uint64_t>(max_entries, e - b);   // a window holds no more records than slots
    // records | result words | the levels of block totals
    Layout lay;
    const size_t o_key = lay.take(32 * m), o_id = lay.take(32 * m), o_ix = lay.take(4 * m), o_cal = lay.take(4 * m);
    const size_t o_out = lay.take(4 * CVU_SNAP_WORDS);
    size_t o_sum[CVD_LEVELS];
    uint64_t w = (e - b + CV_UNIQ_SNAP_BLOCK - 1) / CV_UNIQ_SNAP_BLOCK;
    for (int k = 0; k < CVD_LEVELS; k++) {
        o_sum[k] = lay.take(4 * (size_t)w);
        w = cvd_blocks(w);
    }
    CV_TRY(u->ws.ensure(lay.top + 16));
    uint8_t *base = u->ws.as<uint8_t>();
    hipStream_t s = u->stream;
    auto drain = on_exit([s] { (void)hipStreamSynchronize(s); });
    CvUniqSnap S{};
    S.slot_begin = (uint32_t)b;
    S.slot_end = (uint32_t)e;
    S.max_entries = (uint32_t)max_entries;
    S.key = at<uint32_t>(base, o_key);
    S.id = at<uint32_t>(base, o_id);
    S.index = at<uint32_t>(base, o_ix);
    S.caller = at<uint32_t>(base, o_cal);
    S.out = at<uint32_t>(base, o_out);
    uint32_t *sums[CVD_LEVELS];
    for (int k = 0; k < CVD_LEVELS; k++) sums[k] = at<uint32_t>(base, o_sum[k]);
    CV_TRY(cvk_uniq_snapshot(&u->T, &S, sums, s));
    // the two words first: only the records they count are copied, straight into the caller's arrays
    CV_TRY(hipMemcpyAsync(u->hstat, S.out, 4 * CVU_SNAP_WORDS, hipMemcpyDeviceToHost, s));
    CV_TRY(hipStreamSynchronize(s));
    const size_t cnt = u->hstat[CVU_SNAP_COUNT];
    const uint64_t next = u->hstat[CVU_SNAP_NEXT];
    if (cnt > m || next <= b || next > e) return CV_E_HIP;
    if (cnt) {
        CV_TRY(hipMemcpyAsync(state_key, base + o_key, 32 * cnt, hipMemcpyDeviceToHost, s));
        CV_TRY(hipMemcpyAsync(consumed_id, base + o_id, 32 * cnt, hipMemcpyDeviceToHost, s));
        CV_TRY(hipMemcpyAsync(consumed_index, base + o_ix, 4 * cnt, hipMemcpyDeviceToHost, s));
        CV_TRY(hipMemcpyAsync(consumed_caller, base + o_cal, 4 * cnt, hipMemcpyDeviceToHost, s));
        CV_TRY(hipStreamSynchronize(s));
    }
    drain.armed = false;
    *n = cnt;
    cursor[0] = next == slots ? UINT64_MAX : next;
    cursor[1] = u->epoch;
    return CV_OK;
}

int cv_uniq_clear(cv_uniq *u) {
    if (!u) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(u->mu);
    CV_TRY(hipSetDevice(u->ordinal));
    u->touch();
    CV_TRY(hipMemsetAsync(u->T.occ, 0, 4 * ((size_t)u->T.mask + 1), u->stream));
    CV_TRY(hipStreamSynchronize(u->stream));
    u->resident = 0;
    return CV_OK;
}

int cv_uniq_install(cv_uniq *u, size_t n, const uint8_t *state_key, const uint8_t *consumed_id,
                    const uint32_t *consumed_index, const uint32_t *consumed_caller) {
    if (n == 0) return cv_uniq_clear(u);
    if (!state_key || !consumed_id || !consumed_index || !consumed_caller) return CV_E_ARGS;
    if (n > kUniqMaxStates) return CV_E_TOO_LARGE;
    if (!u) return CV_E_ARGS;
    std::lock_guard<std::mutex> g(u->mu);
    CV_TRY(hipSetDevice(u->ordinal));
    // a fresh table beside the old one, as cv_uniq_reserve builds it: the old one serves until the new one is whole
    const size_t capacity = std::max(u->capacity, n);
    std::random_device rd;
    void *base = nullptr;
    size_t slots = 0;
    int rc = u->alloc(capacity, &base, &slots);
    if (rc != CV_OK) return rc;
    const CvUniqTable to = cvu_carve(base, slots, key_seed(0) ^ rand64(rd));
    rc = uniq_load_into(u, to, n, state_key, consumed_id, consumed_index, consumed_caller);
    if (rc != CV_OK) {
        (void)hipStreamSynchronize(u->stream);
        u->drop(base, slots);                                    // the old table is untouched
        return rc;
    }
    u->adopt(base, slots, capacity);
    u->T = to;
    u->resident = n;
    u->touch();
    return CV_OK;
}

}  // extern "C"
