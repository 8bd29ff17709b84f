// cv_host.h — the engine state every feature of the C-ABI library needs: device and pinned buffers, workspace
// slots, the key pool, the pipeline's outputs, the per-device executors, the context with its options and
// statistics, routing (dispatch), and the short slot and workspace helpers (the longer ones — a slot's stream and
// helper stream, its workspace growth, a verify launch group — serve the core alone and are file-local there).
// Built on cv_stage.h (host staging, no devices) and cv_launch.h (the kernel launchers); included by cv_api.cpp
// (the core) and, through cv_batch.h (what the one-shot batch calls share), by the feature translation units
// cv_api_sign.cpp, cv_api_pmt.cpp, cv_api_uniq.cpp, cv_api_ck.cpp, cv_api_notary.cpp, cv_api_tearoff.cpp and
// cv_api_resolve.cpp.  The types live in namespace cvh (cv_ctx, a global type of the public header, is made of
// them); nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <unordered_map>

// The library is built with hidden host symbols (corda_amd/build.py: -fvisibility=hidden); only the
// entry points the header declares are exported.
#pragma GCC visibility push(default)
#include "../../include/cordaverify.h"
#pragma GCC visibility pop
#include "cv_launch.h"
#include "cv_stage.h"

namespace cvh {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    // slack: allocate 1.25x the request (buffers that grow with the batch); exact sizes for buffers whose
    // caller already sized them (the input ring's blocks)
    hipError_t ensure(size_t bytes, bool slack = true) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(slack ? bytes + bytes / 4 : bytes, 4096);
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        cap = want;
        return hipSuccess;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Pinned (page-locked) host staging buffer: the host-buffer API packs a call's inputs into it so one
// DMA moves them (pageable hipMemcpyAsync stages every copy through the runtime's own buffers — five
// input copies cost ~0.1 ms of a 0.4-0.7 ms notary batch, tools/notary_probe.py).
struct PinBuf {
    void *p = nullptr;
    void *dev = nullptr;   // the device's address of p (hipHostGetDevicePointer)
    size_t cap = 0;
    unsigned flags = hipHostMallocDefault;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = dev = nullptr;
        cap = 0;
        const size_t want = std::max<size_t>(bytes + bytes / 4, 1 << 16);
        hipError_t e = hipHostMalloc(&p, want, flags);
        if (e == hipSuccess && (e = hipHostGetDevicePointer(&dev, p, 0)) != hipSuccess) (void)hipHostFree(p);
        if (e != hipSuccess) {
            p = dev = nullptr;
            return e;
        }
        cap = want;
        return hipSuccess;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
    template <class T> T *dev_as() const { return static_cast<T *>(dev); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = dev = nullptr;
        cap = 0;
    }
};

// Device-resident per-key comb tables (keyed verify), content-addressed by the
// 32 key bytes.  A key's tables are computed once (cv_keyprep_kernel) and reused by every later
// batch on that device; when the pool is full it is emptied (epoch reset) before new keys go in.
struct KeyHash {
    size_t operator()(const std::array<uint8_t, 32> &k) const { return (size_t)key_hash32(k.data()); }
};
struct KeyCache {
    DevBuf ktab, kok, keys, slots, scratch;
    uint32_t cap = 0;
    std::unordered_map<std::array<uint8_t, 32>, uint32_t, KeyHash> map;
    uint64_t hits = 0, misses = 0, resets = 0;
    // the last stream that used the pool and an event after that use (pool_end: what an epoch reset waits
    // for), and the stream of the last table WRITE (keyprep) with an event after it (key_resolve): a reader on
    // another stream waits only for that (pool_begin) — readers do not wait for readers
    hipStream_t last = nullptr;
    hipEvent_t ev = nullptr;
    hipStream_t wlast = nullptr;
    hipEvent_t wev = nullptr;
    // the device-API keyed call's slot_of_key: device copy, pinned staging, event after its upload
    DevBuf slot_of_key;
    PinBuf pin;
    hipEvent_t pin_ev = nullptr;
    bool pin_busy = false;
};

// One verify workspace (per signature: hs 64 B, 2 tables 2 x 1440 B, R record 128 B, ok 1 B, half-size
// digits 292 B) with what orders its use across streams, its drain-overlap helper, and the Merkle leaf
// digests of the sub-chunks that run on it.  A device has kSlots of them: device-API calls on different
// streams take different slots and run concurrently; the host-buffer pipeline deals its sub-chunks
// round-robin over two slots.
struct Slot {
    DevBuf ws_hs, ws_tab, ws_R, ws_ok, ws_dig, mdig;
    uint32_t ws_cap = 0;
    hipStream_t last = nullptr;   // the stream of the last launch group on this workspace
    hipEvent_t ev = nullptr;      // recorded after that group
    uint64_t stamp = 0;           // last use (least-recently-used choice)
    CvkSplit split;               // drain-overlap helper stream + events (created on first need)
    hipStream_t stream = nullptr; // the slot's own stream (slot 0: the device stream)
    PinBuf pin_in;                // small-path staging of one batch: pk | sig | off | len | arena
    DevBuf packed;                // its device copy
    PinBuf pin_head;              // mid-size batches (verify_shard_mid): pk | sig, staged before the range scan
    DevBuf head;                  // its device copy
};
constexpr int kSlots = 4;
constexpr int kPipeSlots = 4;   // most compute slots a pipelined call deals its sub-chunks over (PipeFrame::ns)
// input blocks of the host pipeline on the device: copies run up to kRing sub-chunks ahead of the kernels, so
// a call's copies are all queued early and a Merkle call submitted behind a verify call copies its leaves
// while that verify's kernels run (round 4: with 6 blocks the verify's copies were paced by its kernels and
// the Merkle copies queued behind them, host C3 0.67x of the device rate)
constexpr int kRing = 16;
constexpr int kStage = 6;       // pinned host staging blocks (pageable inputs are packed into them)
constexpr int kOuts = 4;        // pipelined host calls in flight per device (async verify + Merkle calls)
constexpr size_t kFailKeep = 1024;   // failed asynchronous calls remembered per output (PipeOut::failed)
constexpr int kRsVals = 8;           // CV_STATS_RESOLVE values per timed cv_resolve_batch call
constexpr int kTlVals = 14;          // CV_STATS_TIMELINE values per timed call (PipeOut::tl_sum)

// The output of one pipelined host call on one device: its results on the device (dout), the pinned
// copy they come back through, and what pipe_finish copies where.  pending: enqueued, results not yet in
// the caller's arrays; gen counts the calls that used this output.  mu serialises finishing it (cv_wait
// runs without the device lock) against reusing it (under the device lock; order: device -> output).
struct PipeOut {
    std::mutex mu;
    DevBuf dout;
    PinBuf hout;
    // after this call's last launch group on each slot stream, and (Merkle calls) on the copy stream
    hipEvent_t slot_done[kPipeSlots + 1] = {};
    bool slot_used[kPipeSlots + 1] = {};
    bool pending = false;
    uint64_t gen = 0;
    struct Seg {
        void *dst;
        size_t off, len;
    };
    Seg seg[4] = {};
    int nseg = 0;
    // keyed calls: the call's distinct keys and their pool slots on the device (kdev: keys | slot_of_key,
    // uploaded through kstage), the auto path's key_index (pinned, DMAed per sub-chunk)
    DevBuf kdev;
    PinBuf kstage, kidx;
    PinBuf tstage;   // transaction calls: the shard's signature boundaries when the caller's are pageable
    hipEvent_t copied = nullptr;   // after the call's result copies on the output stream (pipe_copy_back)
    // CV_OPT_TIMELINE (synchronous calls): timing events — [0] the first input DMA's start, then per sub-chunk j
    // [1 + 3j] its DMA's end (copy stream), [2 + 3j] its launch group's start, [3 + 3j] its end (slot stream);
    // summarised by pipe_copy_back into tl_sum (the result copies timed on the host there)
    std::vector<hipEvent_t> tl;
    int tl_n = 0;
    size_t tl_first = 0;
    bool tl_ready = false;
    // ramp, last DMA end, span, busy, idle, tail, result copy (ms); first sub-chunk; Merkle-group busy, verify-group
    // busy, last Merkle DMA end (ms); launch groups; host: call entry -> first input DMA enqueued, GPU work joined ->
    // results in the caller's arrays (ms)
    double tl_sum[kTlVals] = {};
    double tl_pre_ms = 0, tl_join_s = 0;
    std::vector<uint8_t> tl_merkle;   // per launch group: 1 = a Merkle group (cv_verify_transactions), 0 = verify
    hipEvent_t tl_ev(size_t k) {
        while (tl.size() <= k) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            tl.push_back(e);
        }
        return tl[k];
    }
    // asynchronous calls on this output whose finish failed: (gen, error), kept after the output is reused so a
    // cv_wait on such a call still returns its error.  Only ticketed calls are recorded (a synchronous call returns
    // its error itself), and a ticket whose call has finished leaves the live map, with its result, at the next
    // ticket_add once 64 are live; so fewer than 64 + kOuts x devices recorded failures can still be needed, and
    // the list keeps kFailKeep (a fixed 64 could evict a live ticket's failure behind failing
    // synchronous calls, and cv_wait then returned CV_OK).
    bool ticketed = false;
    std::deque<std::pair<uint64_t, int>> failed;
    int result_of(uint64_t g) const {
        for (const auto &f : failed)
            if (f.first == g) return f.second;
        return CV_OK;
    }
};

// One persistent thread per device that runs the shards other threads hand it (dispatch), in order.
class DeviceWorker {
  public:
    DeviceWorker() : th_([this] { loop(); }) {}
    ~DeviceWorker() {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_one();
        th_.join();
    }
    void post(std::function<void()> f) {
        {
            std::lock_guard<std::mutex> g(mu_);
            q_.push_back(std::move(f));
        }
        cv_.notify_one();
    }

  private:
    void loop() {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;   // stop requested and nothing left
                f = std::move(q_.front());
                q_.pop_front();
            }
            f();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> q_;
    bool stop_ = false;
    std::thread th_;
};

struct Device {
    int ordinal = 0;
    // mu: held for the whole of a synchronous shard and while an asynchronous one is enqueued; load: the
    // shards in progress or queued on this device (routing); worker: runs shards handed over by dispatch
    std::mutex mu;
    std::atomic<int> load{0};
    std::unique_ptr<DeviceWorker> worker;
    std::mutex worker_mu;   // creation of the worker
    hipStream_t stream = nullptr;
    DevBuf pk, sig, arena, off, len, bitmap, status, seed, tx_begin, digest, ids;
    PinBuf pin_out;                      // small-path verify outputs: bitmap | status
    // zero-copy notary path (verify_shard_small_zc): fine-grained pinned host memory the kernels read
    // (packed records) and store into (verdict nibbles | status) over PCIe
    PinBuf zc_in, zc_out;
    DevBuf pmt;                          // partial Merkle trees: inputs, outputs and workspace, packed
    DevBuf ck;                           // missing signers (cv_api_ck.cpp): inputs, outputs and workspace, packed
    // tear-off verify and signing (cv_api_tearoff.cpp) and cv_resolve_batch (cv_api_resolve.cpp): a call's inputs
    // packed for ONE upload into d.pmt, and the block its outputs come back through
    PinBuf ts_in, ts_out;
    Slot slot[kSlots];
    uint64_t clock = 0;
    KeyCache kc;
    std::unique_ptr<WorkerPool> pool;    // host packing threads (created on the first large host batch)
    // The host pipeline's input ring: sub-chunk j's records go into device block j % kRing by the ONE copy
    // stream (so every H2D copy runs on one DMA queue, never as a blit kernel beside the verify kernels),
    // packed first into the next pinned staging block when the caller's arrays are pageable.  in_ready[q]:
    // after block q's copies (copy stream); in_free[q]: after the kernels that read it (its slot stream);
    // stage_ev[k]: after the copy out of staging block k.
    hipStream_t copy = nullptr;
    hipStream_t outs = nullptr;          // the pipeline's result copies (pipe_finish)
    PipeOut out[kOuts];
    int out_next = 0;
    DevBuf inblk[kRing];
    hipEvent_t in_ready[kRing] = {}, in_free[kRing] = {};
    bool in_used[kRing] = {};
    int ring_next = 0;
    size_t ring_max = 0;                 // the largest ring block (blocks grow to it)
    PinBuf instage[kStage];
    hipEvent_t stage_ev[kStage] = {};
    bool stage_busy[kStage] = {};
    int stage_next = 0;
    // transaction calls: after each Merkle launch group (the signature groups wait for it), + one join event
    std::vector<hipEvent_t> mev;
    // transaction calls with CV_OPT_TXS_MERKLE_STREAM = 2: the stream their Merkle groups run on (created on first
    // use) and those groups' leaf-digest buffer (the groups run one after another on it)
    hipStream_t mstream = nullptr;
    DevBuf mdigest;
    WorkerPool &workers(int threads) {
        if (!pool || pool->threads() != threads) {
            pool.reset();
            pool.reset(new WorkerPool(threads - 1));
        }
        return *pool;
    }
    void post(std::function<void()> f) {
        {
            std::lock_guard<std::mutex> g(worker_mu);
            if (!worker) worker.reset(new DeviceWorker());
        }
        worker->post(std::move(f));
    }
};

// key-table pool capacity per device (keys); 66 KB of tables per key (1.1 GB at the default; the pool
// grows to a call's distinct keys when they exceed it)
constexpr uint32_t kDefaultKeyCap = 1u << 14;
constexpr size_t kKtabBytes = 16512 * 4;  // CV_KTAB_WORDS: 4 comb rows x 129 affine entries x 128 B
constexpr size_t kTabBytes = 9 * 40 * 4;  // CV_TAB_WORDS: k*P, k = 0..8, cached form (cv_verify.h)
// new keys' tables are computed in launches of at most this many keys (bounded keyprep scratch: 270 MB)
constexpr size_t kKeyprepBatch = 4096;

// Verify workspace capacity: batches above it run in chunks of this many signatures (~13.4 GB of
// workspace at 2^22; same-box A/B at 8M signatures: 2^21 73.2, 2^22 72.4, 2^23 72.4 ms -- fewer
// chunk tails to drain; whole-round chunks of 1,966,080 were slower, 73.4 ms).
constexpr uint32_t kVerifyChunk = 1u << 22;

// ---------------------------------------------------------------- options (cv_set_option)
struct OptDesc {
    int64_t def, lo, hi;
};
inline const OptDesc kOpt[CV_OPT_COUNT] = {
    {0, 0, 0},                          // (unused: options start at 1)
    {4096, 0, 1 << 20},                 // CV_OPT_TRI_MAX
    {32768, 0, 1 << 22},                // CV_OPT_QUAD_MAX
    {1, 0, 2},                          // CV_OPT_DRAIN_SPLIT
    {10, 5, 50},                        // CV_OPT_DRAIN_SPLIT_PCT
    {131072, 64, (int64_t)1 << 40},     // CV_OPT_PIPE_MIN
    {32768, 64, 1 << 24},               // CV_OPT_PIPE_FIRST
    {262144, 64, 1 << 24},              // CV_OPT_PIPE_CHUNK
    {196608, 64, 1 << 24},              // CV_OPT_ASYNC_CHUNK (one round of resident waves on MI355X)
    {8, 1, 64},                         // CV_OPT_HOST_THREADS
    {3, 0, 3},                          // CV_OPT_SMALL_ZERO_COPY
    {16384, 1, (int64_t)1 << 40},       // CV_OPT_SMALL_DIRECT_MIN
    {1, 0, 1},                          // CV_OPT_AUTO_KEYED
    {4096, 64, (int64_t)1 << 40},       // CV_OPT_SHARD_MIN
    {262144, 64, (int64_t)1 << 40},     // CV_OPT_SPREAD_MIN
    {262144, 1, 1 << 24},               // CV_OPT_MERKLE_CHUNK
    {32768, 1, (int64_t)1 << 40},       // CV_OPT_PREP_OVERLAP_MIN
    {0, 0, 1},                          // CV_OPT_TIMELINE
    {16, 1, 1024},                      // CV_OPT_PIPE_SPLIT
    {0, 0, 1},                          // CV_OPT_PIPE_OVERLAP_FIRST
    {1, 1, 16},                         // CV_OPT_MID_PIECES
    {2, 2, 4},                          // CV_OPT_PIPE_SLOTS
    {2, 0, 2},                          // CV_OPT_TXS_MERKLE_STREAM
    {0, 0, 4},                          // CV_OPT_FUSED_KEYED (auto lost to the parent in the measurement of DESIGN.md §5.14)
};

// A snapshot of a context's options, taken once per call.
struct Opts {
    CvkPlan plan;
    size_t pipe_min, pipe_first, pipe_chunk, async_chunk, small_direct_min, shard_min, spread_min, merkle_chunk;
    size_t prep_overlap_min;
    size_t pipe_split, mid_pieces, pipe_slots;
    int txs_merkle_stream, fused_keyed;
    int threads, small_zc, auto_keyed, timeline, pipe_overlap_first;
};

// host-side time of the pipelined path (cv_diag_stats CV_STATS_PIPE), of the zero-copy small path
// (CV_STATS_SMALL) and the routing counters (CV_STATS_ROUTE)
struct Stats {
    double pipe[5] = {};   // plan, pack, wait, enqueue, sync (seconds)
    uint64_t pipe_calls = 0, pipe_chunks = 0, pipe_direct = 0;
    double small[5] = {};  // plan + setup, pack, launch, sync, assemble
    uint64_t small_calls = 0;
    uint64_t calls = 0, routed_whole = 0, split_calls = 0, shards = 0, keyed_calls = 0, keyed_chunks = 0,
             merkle_calls = 0, merkle_chunks = 0;
    double tl[kTlVals + 1] = {};   // CV_STATS_TIMELINE sums (PipeOut::tl_sum) + calls
    double rs[kRsVals + 1] = {};   // CV_STATS_RESOLVE sums + calls
};

inline int hip_rc(hipError_t e) {
    if (e == hipSuccess) return CV_OK;
    if (e == hipErrorOutOfMemory) return CV_E_OOM;
    return CV_E_HIP;
}

#define CV_TRY(expr)                        \
    do {                                    \
        hipError_t e_ = (expr);             \
        if (e_ != hipSuccess) return hip_rc(e_); \
    } while (0)

// Runs fn at scope exit unless dismissed (error paths that must drain queued DMAs out of pinned
// staging before a later call reuses or frees it).
template <class F> struct OnExit {
    F fn;
    bool armed = true;
    ~OnExit() {
        if (armed) fn();
    }
};
template <class F> OnExit<F> on_exit(F fn) { return OnExit<F>{fn}; }

inline hipError_t slot_events(Slot &sl) {
    hipError_t e = hipSuccess;
    if (!sl.ev && (e = hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming)) != hipSuccess) return e;
    return e;
}

// The workspace slot for a launch group on stream s: the slot s used last (no cross-stream wait),
// else the least recently used one (ws_begin then waits for that slot's previous group).
inline Slot &pick_slot(Device &d, hipStream_t s) {
    for (Slot &sl : d.slot)
        if (sl.last == s) return sl;
    Slot *best = &d.slot[0];
    for (Slot &sl : d.slot)
        if (sl.stamp < best->stamp) best = &sl;
    return *best;
}

// Every use of a shared device resource (a workspace slot, the key pool) is ordered across streams:
// a launch group enqueued on stream s first waits for the previous group when that ran on another
// stream (ws_begin), and marks its own end (ws_end).  Device-pointer calls may therefore be made on any
// streams; two streams that hold different slots run concurrently, and a stream that takes over a slot
// waits for it instead of racing on it.  Callers hold the device lock around ws_begin .. ws_end.
inline hipError_t ws_begin(Device &d, Slot &sl, hipStream_t s) {
    hipError_t e = slot_events(sl);
    if (e != hipSuccess) return e;
    sl.stamp = ++d.clock;
    if (sl.last && sl.last != s) e = hipStreamWaitEvent(s, sl.ev, 0);
    return e;
}
inline hipError_t ws_end(Slot &sl, hipStream_t s) {
    sl.last = s;
    return hipEventRecord(sl.ev, s);
}
inline hipError_t pool_begin(KeyCache &kc, hipStream_t s) {
    hipError_t e = hipSuccess;
    if (!kc.ev && (e = hipEventCreateWithFlags(&kc.ev, hipEventDisableTiming)) != hipSuccess) return e;
    if (!kc.wev && (e = hipEventCreateWithFlags(&kc.wev, hipEventDisableTiming)) != hipSuccess) return e;
    if (kc.wlast && kc.wlast != s) e = hipStreamWaitEvent(s, kc.wev, 0);
    return e;
}
inline hipError_t pool_end(KeyCache &kc, hipStream_t s) {
    kc.last = s;
    return hipEventRecord(kc.ev, s);
}

}  // namespace cvh

struct cv_ctx {
    std::vector<std::unique_ptr<cvh::Device>> devs;
    std::atomic<int64_t> opt[CV_OPT_COUNT];
    std::atomic<uint32_t> key_cap{cvh::kDefaultKeyCap};
    std::atomic<uint32_t> rr{0};            // routing: where the search for the least loaded device starts
    // asynchronous calls: ticket -> (device index, output index, that output's gen) per shard
    std::mutex tk_mu;
    uint64_t next_ticket = 0;
    std::unordered_map<uint64_t, std::vector<std::array<uint64_t, 3>>> tickets;
    std::map<uint64_t, int> tickets_done;   // finished tickets pruned from `tickets`, with their result
    std::mutex st_mu;
    cvh::Stats stats;
    cv_ctx() {
        for (int k = 0; k < CV_OPT_COUNT; k++) opt[k].store(cvh::kOpt[k].def);
    }
    cvh::Opts opts() const {
        cvh::Opts o;
        o.plan.tri_max = (uint32_t)opt[CV_OPT_TRI_MAX].load();
        o.plan.quad_max = (uint32_t)opt[CV_OPT_QUAD_MAX].load();
        o.plan.split = (int)opt[CV_OPT_DRAIN_SPLIT].load();
        o.plan.split_pct = (int)opt[CV_OPT_DRAIN_SPLIT_PCT].load();
        o.pipe_min = (size_t)opt[CV_OPT_PIPE_MIN].load();
        o.pipe_first = (size_t)opt[CV_OPT_PIPE_FIRST].load() / 64 * 64;
        o.pipe_chunk = (size_t)opt[CV_OPT_PIPE_CHUNK].load() / 64 * 64;
        o.async_chunk = (size_t)opt[CV_OPT_ASYNC_CHUNK].load() / 64 * 64;
        o.threads = (int)opt[CV_OPT_HOST_THREADS].load();
        o.small_zc = (int)opt[CV_OPT_SMALL_ZERO_COPY].load();
        o.small_direct_min = (size_t)opt[CV_OPT_SMALL_DIRECT_MIN].load();
        o.auto_keyed = (int)opt[CV_OPT_AUTO_KEYED].load();
        o.shard_min = (size_t)opt[CV_OPT_SHARD_MIN].load();
        o.spread_min = (size_t)opt[CV_OPT_SPREAD_MIN].load();
        o.merkle_chunk = (size_t)opt[CV_OPT_MERKLE_CHUNK].load();
        o.prep_overlap_min = (size_t)opt[CV_OPT_PREP_OVERLAP_MIN].load();
        o.timeline = (int)opt[CV_OPT_TIMELINE].load();
        o.pipe_split = (size_t)opt[CV_OPT_PIPE_SPLIT].load();
        o.pipe_overlap_first = (int)opt[CV_OPT_PIPE_OVERLAP_FIRST].load();
        o.mid_pieces = (size_t)opt[CV_OPT_MID_PIECES].load();
        o.pipe_slots = (size_t)opt[CV_OPT_PIPE_SLOTS].load();
        o.txs_merkle_stream = (int)opt[CV_OPT_TXS_MERKLE_STREAM].load();
        o.fused_keyed = (int)opt[CV_OPT_FUSED_KEYED].load();
        return o;
    }
};

// The fixed-key signer (cv_api_sign.cpp): one Ed25519 key expanded once per device of the context; rec[k] is device
// k's record (a | prefix | abyte, CVK_SIGN_REC_BYTES), in the order of ctx->devs.  Immutable after cv_signer_open, so
// any number of threads sign with it at once; the only host copy of key material is the public key.
struct cv_signer {
    cv_ctx *ctx = nullptr;
    std::vector<void *> rec;
    uint8_t pk[32] = {};
};

namespace cvh {

constexpr size_t kUniqMaxStates = (size_t)1 << 30;   // a table's slot count stays within 2^31

inline uint64_t rand64(std::random_device &rd) { return ((uint64_t)rd() << 32) | rd(); }

// The host frame of a device-resident table (cv_table.h): what the uniqueness set and the key store share.  It lives
// on one device of its context, with a stream, a workspace and a pinned read-back block of its own, so its calls take
// no device lock: they serialise on the mutex.  The table is ONE allocation of slots * slot_bytes with occ first, the
// slot count cv_table_slots(capacity, 16); its owner carves it (cvu_carve, cks_carve) and keeps the seed.  Words
// CVT_D_ERROR and CVT_D_MAXPROBE of the stat_words device counters are folded here, the rest by the owner.
struct Resident {
    cv_ctx *ctx = nullptr;
    int ordinal = 0;
    std::mutex mu;
    hipStream_t stream = nullptr;
    void *tab = nullptr;
    size_t slots = 0, slot_bytes = 0;
    size_t capacity = 0, resident = 0;
    DevBuf ws, dstat;
    uint32_t *hstat = nullptr;               // pinned: the device counters read back
    size_t stat_words = 0;
    uint64_t last_probe = 0;
    bool wipe = false;                       // overwrite a table before freeing it (the store: it holds private keys)

    // the open entry points' checks, in their order
    template <class H> static int open_check(cv_ctx *c, int device, size_t cap, H **out) {
        if (out) *out = nullptr;
        if (!c || !out || device < 0 || (size_t)device >= c->devs.size()) return CV_E_ARGS;
        return cap > kUniqMaxStates ? CV_E_TOO_LARGE : CV_OK;
    }
    // a fresh, empty table for `cap` entries on the current device: occ zeroed on the stream, the rest is written
    // before it is read
    int alloc(size_t cap, void **base, size_t *nslots) {
        const size_t n = (size_t)cv_table_slots(cap, 16);
        void *p = nullptr;
        CV_TRY(hipMalloc(&p, slot_bytes * n));
        const hipError_t e = hipMemsetAsync(p, 0, 4 * n, stream);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return hip_rc(e);
        }
        *base = p;
        *nslots = n;
        return CV_OK;
    }
    void drop(void *base, size_t nslots) {
        if (!base) return;
        if (wipe && stream) {
            (void)hipMemsetAsync(base, 0, slot_bytes * nslots, stream);
            (void)hipStreamSynchronize(stream);
        }
        (void)hipFree(base);
    }
    void adopt(void *base, size_t nslots, size_t cap) {
        drop(tab, slots);
        tab = base;
        slots = nslots;
        capacity = cap;
    }
    // after open_check; a failure leaves what was made so far to close()
    int open(cv_ctx *c, int device, size_t cap, size_t sbytes, size_t swords, bool wipe_tables) {
        ctx = c;
        ordinal = c->devs[(size_t)device]->ordinal;
        capacity = std::max<size_t>(cap, 1);
        slot_bytes = sbytes;
        stat_words = swords;
        wipe = wipe_tables;
        CV_TRY(hipSetDevice(ordinal));
        CV_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        CV_TRY(hipHostMalloc(reinterpret_cast<void **>(&hstat), 4 * stat_words, hipHostMallocDefault));
        CV_TRY(dstat.ensure(4 * stat_words, false));
        const int rc = alloc(capacity, &tab, &slots);
        if (rc != CV_OK) return rc;
        CV_TRY(hipStreamSynchronize(stream));
        return CV_OK;
    }
    // release_own: the owner's buffers, released where they always were: behind the table and the workspace, ahead
    // of the counters and the stream
    template <class Own> void close(Own release_own) {
        (void)hipSetDevice(ordinal);
        if (stream) (void)hipStreamSynchronize(stream);
        drop(tab, slots);
        tab = nullptr;
        ws.release();
        release_own();
        dstat.release();
        if (hstat) (void)hipHostFree(hstat);
        if (stream) (void)hipStreamDestroy(stream);
        hstat = nullptr, stream = nullptr;
    }
    // counters zeroed before a call's kernels / read back (a synchronisation) and folded after them
    int stat_begin() {
        CV_TRY(hipMemsetAsync(dstat.p, 0, 4 * stat_words, stream));
        return CV_OK;
    }
    int stat_read() {
        hipError_t e = hipMemcpyAsync(hstat, dstat.p, 4 * stat_words, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) std::memset(hstat, 0, 4 * stat_words);   // nothing for the owner's folds to add
        return hip_rc(e);
    }
    int stat_end() {
        const int rc = stat_read();
        if (rc != CV_OK) return rc;
        last_probe = hstat[CVT_D_MAXPROBE];
        return hstat[CVT_D_ERROR] ? CV_E_HIP : CV_OK;         // a probe ran out of slots: never with these sizes
    }
    // Growth to `cap` entries (never shrinks), the caller holding mu: a fresh table, rehash(base, slots) — the
    // owner's launcher from the old table into the new one — between stat_begin and end(), the owner's stat end (the
    // frame's, or one that folds more); the swap on success, and on failure the new table dropped and the old one
    // untouched.  *rehashed says whether tab is a new table now (false: nothing to do, or the slots already held it).
    template <class Rehash, class End> int grow(size_t cap, Rehash rehash, End end, bool *rehashed) {
        *rehashed = false;
        if (cap <= capacity) return CV_OK;
        CV_TRY(hipSetDevice(ordinal));
        if ((size_t)cv_table_slots(cap, 16) == slots) {          // the slots already hold it
            capacity = cap;
            return CV_OK;
        }
        void *base = nullptr;
        size_t nslots = 0;
        int rc = alloc(cap, &base, &nslots);
        if (rc != CV_OK) return rc;
        rc = stat_begin();
        if (rc == CV_OK) rc = hip_rc(rehash(base, nslots));
        const int rc2 = end();                                   // synchronises, also after a failed launch
        if (rc == CV_OK) rc = rc2;
        if (rc != CV_OK) {
            drop(base, nslots);
            return rc;
        }
        adopt(base, nslots, cap);
        *rehashed = true;
        return CV_OK;
    }
};

}  // namespace cvh

// The uniqueness set (cv_api_uniq.cpp): a resident frame (its mutex is the reference's ThreadBox) whose table is five
// arrays (occ | key | id | index | caller, cv_uniq.h); growth builds a second one, rehashes on the device and frees
// the first.
struct cv_uniq : cvh::Resident {
    CvUniqTable T{};
    int max_rounds = 8;
    uint64_t last_rounds = 0, last_tail = 0, wraps = 0;
    // advanced by every call that may change the table's contents or layout (commit, load, install, clear, a reserve
    // that rehashes); a snapshot cursor carries the value of the call that started its pass.  Never 0.
    uint64_t epoch = 1;
    void touch() {
        if (++epoch == 0) epoch = 1;
    }
    // cv_notarise_batch (cv_api_notary.cpp): its inputs packed in pinned memory for one upload, its device copy of them
    // with the pipeline's workspace and outputs behind, and the pinned block the outputs come back through
    cvh::PinBuf nin, nout;
    cvh::DevBuf nws;
    std::unique_ptr<cvh::WorkerPool> pool;   // host threads that pack a large batch's inputs (created on the first one)
};

namespace cvh {

// cv_api_uniq.cpp, shared with cv_api_notary.cpp: the frame's stat_end with the set's wraps folded, the slots of a
// batch's table of state indices, the decision itself
int uniq_stat_end(cv_uniq *u);
inline size_t uniq_bslots(size_t nstates) { return (size_t)cv_table_slots(nstates, 16); }
int uniq_decide(cv_uniq *u, const CvUniqBatch &B, uint32_t *cur, uint32_t *nxt, uint64_t *rounds);

// cv_api.cpp: one verify launch group of n signatures (device pointers, as cv_ed25519_verify_device) on stream s of
// device d, ordered on the shared verify workspace; the caller holds d.mu
hipError_t verify_device_locked(cv_ctx *ctx, Device &d, size_t n, const uint8_t *pk, const uint8_t *sig,
                                const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint64_t *bitmap,
                                uint8_t *status, hipStream_t s);
// cv_api.cpp: the keyed verify of n signatures on stream s of device d — the body of cv_ed25519_verify_device_keyed,
// for it and for the fused batch calls: the nkeys distinct keys resolved against d's key pool from their host copy
// hkeys (pool_begin, key_resolve, the slot_of_key upload), cvk_verify_keyed over the device pointers, pool_end.  The
// caller holds d.mu (cv_resolve_batch through dispatch_one; cv_notarise_batch takes it under its set's mutex).
// phase_ms as cv_ed25519_verify_device_keyed's; an error leaves nothing queued on s.
int verify_keyed_locked(cv_ctx *ctx, Device &d, size_t n, size_t nkeys, const uint8_t *hkeys, const uint8_t *d_keys,
                        const uint32_t *d_key_index, const uint8_t *sig, const uint8_t *arena, const uint64_t *off,
                        const uint32_t *len, uint64_t *bitmap, uint8_t *status, hipStream_t s, float *phase_ms);
// cv_api_hotkeys.cpp: the hot-key route (cv_hotkeys.h) in its two halves, for cv_ed25519_verify_device_hotkeys and the
// fused batch calls.  hotkeys_front enqueues on s the dedupe over H.pk, the route's steps up to the records' scan and
// the copy of head | `rows` hot key rows (cvh_rows) to `host`; it takes no lock and synchronises nothing.  Once that
// copy has arrived — the route's one synchronisation, the caller's — verify_hotkeys_locked decides from it and
// enqueues the rest: verify_device_locked over the caller's arrays when no key is hot, verify_keyed_locked over them
// when every key is, else the gather (it reads H.off / H.len: behind whatever writes them), both over their
// sub-batches and the merge into bitmap / status (optional).  route_out (optional) = {nkeys, hot keys, hot records,
// cold records}.  The caller holds d.mu; CV_E_HIP after a probe error of the dedupe.
hipError_t hotkeys_front(const CvHot &H, const CvhLayout &L, void *ws, uint64_t seed, size_t rows, void *host,
                         hipStream_t s);
int verify_hotkeys_locked(cv_ctx *ctx, Device &d, const CvHot &H, size_t rows, const void *host, const uint8_t *arena,
                          uint64_t *bitmap, uint8_t *status, hipStream_t s, uint32_t route_out[4]);

inline Device *find_dev(cv_ctx *ctx, int device) {
    for (auto &d : ctx->devs)
        if (d->ordinal == device) return d.get();
    return nullptr;
}

// the index of device d in its context (the order of ctx->devs)
inline size_t dev_index(cv_ctx *ctx, const Device &d) {
    for (size_t k = 0; k < ctx->devs.size(); k++)
        if (ctx->devs[k].get() == &d) return k;
    return 0;
}

// ---------------------------------------------------------------- routing (dispatch)
// Runs fn(device, b, e, packing threads) over shards of [0, n) and returns the first error.  The shard
// plan ("Routing and threading"):
//   - one device, or n <= shard_min: the whole batch on ONE device — the least loaded (shards in progress
//     or queued on it), ties broken by a rotating start, so concurrent notary batches land on different
//     GPUs instead of each being cut eight ways (a shard below the tri-chain size costs the kernel
//     chain's floor, ~0.22 ms, whatever its size);
//   - n >= spread_min: contiguous shards over ALL devices (a throughput batch);
//   - between: over the devices idle at submission, at most ceil(n / shard_min) of them, at least one
//     (the least loaded) — a lone caller's mid-size batch spreads, a loaded node's does not.
// Shard starts are multiples of `align` (64 for verify: whole bitmap words).  The caller's thread runs
// the first shard; the others go to their devices' workers.  A shard runs under its device's lock;
// nothing holds a lock while waiting for another, so concurrent calls cannot deadlock.
template <class F>
inline int dispatch(cv_ctx *ctx, const Opts &o, size_t n, size_t align, F fn) {
    const size_t ndev = ctx->devs.size();
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int threads = (int)std::max<size_t>(1, std::min<size_t>((size_t)o.threads, std::max<size_t>(1, hw / ndev)));
    std::vector<size_t> pick;
    const uint32_t start = ctx->rr.fetch_add(1);
    if (ndev == 1) {
        pick.push_back(0);
    } else if (n >= o.spread_min) {
        for (size_t k = 0; k < ndev; k++) pick.push_back(k);
    } else {
        const size_t kmax = n <= o.shard_min ? 1 : (n + o.shard_min - 1) / o.shard_min;
        for (size_t j = 0; j < ndev && pick.size() < kmax; j++) {
            const size_t k = (start + j) % ndev;
            if (ctx->devs[k]->load.load() == 0) pick.push_back(k);
        }
        if (pick.empty()) {
            size_t best = start % ndev;
            for (size_t j = 0; j < ndev; j++) {
                const size_t k = (start + j) % ndev;
                if (ctx->devs[k]->load.load() < ctx->devs[best]->load.load()) best = k;
            }
            pick.push_back(best);
        }
    }
    const size_t ns = pick.size();
    size_t per = (n + ns - 1) / ns;
    per = (per + align - 1) / align * align;
    struct ShardPart {
        size_t dev, b, e;
    };
    std::vector<ShardPart> parts;
    for (size_t j = 0; j < ns; j++) {
        const size_t b = std::min(n, j * per), e = std::min(n, b + per);
        if (b < e || j == 0) parts.push_back({pick[j], b, e});
    }
    {
        std::lock_guard<std::mutex> g(ctx->st_mu);
        ctx->stats.calls++;
        ctx->stats.shards += parts.size();
        if (parts.size() == 1) ctx->stats.routed_whole++;
        else ctx->stats.split_calls++;
    }
    for (const ShardPart &p : parts) ctx->devs[p.dev]->load.fetch_add(1);
    std::vector<int> rc(parts.size(), CV_OK);
    auto run = [&](size_t j) {
        Device &d = *ctx->devs[parts[j].dev];
        {
            std::lock_guard<std::mutex> g(d.mu);
            rc[j] = fn(d, parts[j].b, parts[j].e, threads);
        }
        d.load.fetch_sub(1);
    };
    if (parts.size() == 1) {
        run(0);
        return rc[0];
    }
    std::mutex m;
    std::condition_variable cv;
    size_t left = parts.size() - 1;
    for (size_t j = 1; j < parts.size(); j++)
        ctx->devs[parts[j].dev]->post([&, j] {
            run(j);
            std::lock_guard<std::mutex> g(m);
            if (--left == 0) cv.notify_one();
        });
    run(0);
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return left == 0; });
    }
    for (int r : rc)
        if (r != CV_OK) return r;
    return CV_OK;
}

}  // namespace cvh
