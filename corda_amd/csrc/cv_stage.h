// cv_stage.h — host-side staging logic of the C-ABI library that knows neither devices nor contexts: the packing
// thread pool, the staging layouts of record and Merkle ranges (plan, bounds, pack, direct DMA), the key dedupe and
// the sub-chunk planners.  Included by cv_host.h (the engine state) and, on its own, by host-only tools and tests
// (tools/microbench/gate_bench.cpp).  Everything here is defined once, inline, in namespace cvh.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

namespace cvh {

inline double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// A fixed set of host threads for index-parallel jobs (the host-buffer path's packing, range scans and key
// dedupe): run(ntasks, fn) calls fn(i) for every i in [0, ntasks) on the helpers and the calling thread and
// returns when all are done.  One per device, used under the device lock.
class WorkerPool {
  public:
    explicit WorkerPool(int helpers) {
        for (int t = 0; t < helpers; t++) th_.emplace_back([this] { loop(); });
    }
    ~WorkerPool() {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    int threads() const { return (int)th_.size() + 1; }
    // The caller works through the tasks too and returns once every task is done and every helper that
    // joined has left: helpers still asleep are not waited for (their wake-up, 10-30 us, used to be on
    // every call's critical path), and one that wakes after the run finds no job and sleeps again.
    void run(size_t ntasks, const std::function<void(size_t)> &fn) {
        if (ntasks == 0) return;
        if (th_.empty() || ntasks == 1) {
            for (size_t i = 0; i < ntasks; i++) fn(i);
            return;
        }
        {
            std::lock_guard<std::mutex> g(mu_);
            job_ = &fn;
            ntasks_ = ntasks;
            next_.store(0);
            done_.store(0);
            gen_++;
        }
        cv_.notify_all();
        drain(fn, ntasks);
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [&] { return active_ == 0 && done_.load() == ntasks; });
        job_ = nullptr;
    }

  private:
    void drain(const std::function<void(size_t)> &fn, size_t ntasks) {
        for (size_t i; (i = next_.fetch_add(1)) < ntasks;) {
            fn(i);
            done_.fetch_add(1);
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(size_t)> *job;
            size_t ntasks;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                if (!job_) continue;   // that run is over
                job = job_;
                ntasks = ntasks_;
                active_++;
            }
            drain(*job, ntasks);
            {
                std::lock_guard<std::mutex> g(mu_);
                if (--active_ == 0) done_cv_.notify_one();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    const std::function<void(size_t)> *job_ = nullptr;
    size_t ntasks_ = 0, active_ = 0;
    std::atomic<size_t> next_{0}, done_{0};
    uint64_t gen_ = 0;
    bool stop_ = false;
};

// ---------------------------------------------------------------- host staging
inline size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

// Host copies into pinned staging.  A large copy is done by the device's worker pool (one core copies
// ~10-12 GB/s, below what the DMA takes): each segment is cut into 256 KB pieces the workers take in
// turn.  Copies below par_min in all, 1 MB unless the caller says otherwise, stay on the calling thread (a notary
// batch: waking workers costs more).
struct CopyJob {
    void *dst;
    const void *src;
    size_t len;
};
inline void par_copy(const std::vector<CopyJob> &jobs, WorkerPool *pool, size_t par_min = (size_t)1 << 20) {
    constexpr size_t kPiece = 256 * 1024;
    size_t total = 0;
    for (const CopyJob &j : jobs) total += j.len;
    if (!pool || pool->threads() <= 1 || total < par_min) {
        for (const CopyJob &j : jobs)
            if (j.len) std::memcpy(j.dst, j.src, j.len);
        return;
    }
    std::vector<CopyJob> pieces;
    pieces.reserve(total / kPiece + jobs.size());
    for (const CopyJob &j : jobs)
        for (size_t o = 0; o < j.len; o += kPiece)
            pieces.push_back({static_cast<uint8_t *>(j.dst) + o, static_cast<const uint8_t *>(j.src) + o,
                              std::min(kPiece, j.len - o)});
    pool->run(pieces.size(), [&pieces](size_t k) { std::memcpy(pieces[k].dst, pieces[k].src, pieces[k].len); });
}

// The byte range [lo, hi) of records [b, e) in an arena (min offset, max end) and their total bytes; the
// scan runs in slices of 64K records over the pool.
struct Span {
    uint64_t lo = UINT64_MAX, hi = 0, bytes = 0;
};
// One slice of arena_span.  The unsigned 64-bit min / max vectorise only with AVX2 (the x86-64 baseline has
// no 64-bit compare): the AVX2 instance runs where the CPU has it (65,536 records: 150 -> 48 us on one core
// of this build host).  Dispatched by a cached cpuid test rather than target_clones, whose load-time resolver
// runs before ThreadSanitizer's runtime is up (tests/sanitize).
template <int> inline void span_slice_impl(size_t i0, size_t i1, const uint64_t *off, const uint32_t *len,
                                           uint64_t *out) {
    uint64_t lo = UINT64_MAX, hi = 0, bytes = 0;
    for (size_t i = i0; i < i1; i++) {
        uint64_t end = off[i] + len[i];
        end |= -(uint64_t)(end < off[i]);   // a record whose end wraps saturates: never "in bounds"
        lo = std::min<uint64_t>(lo, off[i]);
        hi = std::max<uint64_t>(hi, end);
        bytes += len[i];
    }
    out[0] = lo;
    out[1] = hi;
    out[2] = bytes;
}
__attribute__((target("avx2"))) inline void span_slice_avx2(size_t i0, size_t i1, const uint64_t *off,
                                                            const uint32_t *len, uint64_t *out) {
    span_slice_impl<1>(i0, i1, off, len, out);
}
inline void span_slice(size_t i0, size_t i1, const uint64_t *off, const uint32_t *len, uint64_t *out) {
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2)
        span_slice_avx2(i0, i1, off, len, out);
    else
        span_slice_impl<0>(i0, i1, off, len, out);
}
inline Span arena_span(size_t b, size_t e, const uint64_t *off, const uint32_t *len, WorkerPool *pool) {
    // with a pool: slices of 8,192 records (the pipeline's sub-chunks: their scans precede their packing on
    // the call's critical path); without, one thread (AVX2)
    const size_t kSlice = pool ? 8192 : 65536;
    const size_t nslices = (e - b + kSlice - 1) / kSlice;
    std::vector<Span> part(std::max<size_t>(nslices, 1));
    auto scan = [&](size_t k) {
        uint64_t r[3];
        span_slice(b + k * kSlice, std::min(e, b + (k + 1) * kSlice), off, len, r);
        part[k].lo = r[0];
        part[k].hi = r[1];
        part[k].bytes = r[2];
    };
    if (pool && nslices > 1)
        pool->run(nslices, scan);
    else
        for (size_t k = 0; k < nslices; k++) scan(k);
    Span s;
    for (const Span &r : part) {
        s.lo = std::min(s.lo, r.lo);
        s.hi = std::max(s.hi, r.hi);
        s.bytes += r.bytes;
    }
    if (s.hi < s.lo) s.lo = s.hi = 0;
    return s;
}

// Staging layout of signature records [b, e): pk | kidx | sig | off | len | arena, 16-B aligned parts (pk
// absent in keyed staging, kidx present only there).  The arena part is the byte range [lo, hi) the records'
// messages span, with lo rounded down to 16 so the device arena pointer keeps every message's alignment;
// the kernels get arena_dev - lo and the caller's offsets unchanged.  When the messages are scattered (the
// range is more than twice their bytes + 1 MB), they are gathered back to back instead and the offsets
// rewritten ("compact").
struct Stage {
    size_t n = 0, o_pk = 0, o_kidx = 0, o_sig = 0, o_off = 0, o_len = 0, o_ar = 0, total = 0;
    uint64_t lo = 0, hi = 0;
    uint64_t extent = 0;   // max(off + len) over the records, whatever the layout (UINT64_MAX: an end wrapped)
    bool compact = false, keyed = false;
};
inline Stage stage_plan(size_t b, size_t e, const uint64_t *off, const uint32_t *len, WorkerPool *pool = nullptr,
                        bool keyed = false) {
    Stage st;
    st.n = e - b;
    st.keyed = keyed;
    const Span sp = arena_span(b, e, off, len, pool);
    const uint64_t lo = sp.lo & ~(uint64_t)15;
    st.compact = sp.hi - lo > 2 * sp.bytes + (1u << 20);
    st.lo = st.compact ? 0 : lo;
    st.hi = st.compact ? sp.bytes : sp.hi;
    st.extent = sp.hi;
    const size_t n = st.n;
    st.o_pk = 0;
    st.o_kidx = keyed ? 0 : al16(n * 32);
    st.o_sig = st.o_kidx + (keyed ? al16(n * 4) : 0);
    st.o_off = st.o_sig + al16(n * 64);
    st.o_len = st.o_off + al16(n * 8);
    st.o_ar = st.o_len + al16(n * 4);
    st.total = st.o_ar + al16(st.hi - st.lo + 16);
    return st;
}
// The records of a stage end inside the caller's arena of arena_bytes (UINT64_MAX: no bound given) and no
// record's off + len wraps.  Checked on the true extent, not on [lo, hi): a compacted stage's hi is the SUM of
// its message lengths, which says nothing about where the scattered records lie.
inline bool stage_in_bounds(const Stage &st, uint64_t arena_bytes) {
    return st.extent != UINT64_MAX && st.extent <= arena_bytes;
}
// Packs records [b, e) into h by the plan (keys / key indices + signatures first: `first_part` runs after
// them, so their DMA can start while the rest is packed).
inline void stage_pack_tail(const Stage &st, uint8_t *h, size_t b, const uint8_t *arena, const uint64_t *off,
                            const uint32_t *len, WorkerPool *pool);
template <class F>
inline void stage_pack(const Stage &st, uint8_t *h, size_t b, const uint8_t *pk, const uint32_t *kidx,
                       const uint8_t *sig, const uint8_t *arena, const uint64_t *off, const uint32_t *len,
                       WorkerPool *pool, F first_part) {
    const size_t n = st.n;
    if (st.keyed)
        par_copy({{h + st.o_kidx, kidx + b, n * 4}, {h + st.o_sig, sig + b * 64, n * 64}}, pool);
    else
        par_copy({{h + st.o_pk, pk + b * 32, n * 32}, {h + st.o_sig, sig + b * 64, n * 64}}, pool);
    first_part();
    stage_pack_tail(st, h, b, arena, off, len, pool);
}
// The offsets, lengths and message bytes of a stage (its parts from o_off on).
inline void stage_pack_tail(const Stage &st, uint8_t *h, size_t b, const uint8_t *arena, const uint64_t *off,
                            const uint32_t *len, WorkerPool *pool) {
    const size_t n = st.n;
    uint64_t *hoff = reinterpret_cast<uint64_t *>(h + st.o_off);
    uint8_t *har = h + st.o_ar;
    if (st.compact) {
        par_copy({{h + st.o_len, len + b, n * 4}}, nullptr);
        uint64_t pos = 0;
        for (size_t i = 0; i < n; i++) {
            hoff[i] = pos;
            if (len[b + i]) std::memcpy(har + pos, arena + off[b + i], len[b + i]);
            pos += len[b + i];
        }
    } else {
        par_copy({{h + st.o_off, off + b, n * 8}, {h + st.o_len, len + b, n * 4},
                  {har, st.hi > st.lo ? arena + st.lo : nullptr, (size_t)(st.hi - st.lo)}},
                 pool);
    }
    std::memset(har + (st.hi - st.lo), 0, 16);
}

// Is [p, p + bytes) page-locked host memory (hipHostMalloc / hipHostRegister)?  Both ends are looked
// up; a failed lookup (pageable memory) clears the runtime's last-error state so no later
// hipGetLastError reports it.
inline bool host_pinned(const void *p, size_t bytes) {
    if (!p || bytes == 0) return p != nullptr;
    const uint8_t *q[2] = {static_cast<const uint8_t *>(p), static_cast<const uint8_t *>(p) + bytes - 1};
    for (const uint8_t *x : q) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, x) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        if (a.type != hipMemoryTypeHost) return false;
    }
    return true;
}
// Direct form of a stage: the record arrays of [b, e) and the arena range all pinned (and the arena
// not compacted), so they can be DMAed from where they are.
inline bool stage_direct(const Stage &st, size_t b, const uint8_t *pk, const uint32_t *kidx, const uint8_t *sig,
                         const uint8_t *arena, const uint64_t *off, const uint32_t *len) {
    if (st.compact) return false;
    const size_t n = st.n;
    return (st.keyed ? host_pinned(kidx + b, n * 4) : host_pinned(pk + b * 32, n * 32)) &&
           host_pinned(sig + b * 64, n * 64) && host_pinned(off + b, n * 8) && host_pinned(len + b, n * 4) &&
           (st.hi == st.lo || host_pinned(arena + st.lo, st.hi - st.lo));
}
// The stage's DMAs straight from the caller's pinned arrays into the device block dv (the layout of
// stage_pack).  The 16 bytes after the arena part keep whatever the block held: the kernels read a
// message only through dword windows clamped to its last byte and mask the bytes past it, so those
// bytes never reach a verdict — and a fill there would be a blit KERNEL on the copy queue, which waits
// for a free CU slot behind the running verify waves (it held the C2 copy stream for 2.5 ms,
// profiles/r03d_timeline_pinned.txt).
inline hipError_t stage_dma_direct(const Stage &st, uint8_t *dv, size_t b, const uint8_t *pk, const uint32_t *kidx,
                                   const uint8_t *sig, const uint8_t *arena, const uint64_t *off, const uint32_t *len,
                                   hipStream_t s) {
    const size_t n = st.n;
    hipError_t e = st.keyed ? hipMemcpyAsync(dv + st.o_kidx, kidx + b, n * 4, hipMemcpyHostToDevice, s)
                            : hipMemcpyAsync(dv + st.o_pk, pk + b * 32, n * 32, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dv + st.o_sig, sig + b * 64, n * 64, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dv + st.o_off, off + b, n * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dv + st.o_len, len + b, n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && st.hi > st.lo)
        e = hipMemcpyAsync(dv + st.o_ar, arena + st.lo, st.hi - st.lo, hipMemcpyHostToDevice, s);
    return e;
}

// Staging layout of Merkle transactions [t0, t1) with leaves [l0, l1): off | len | tx_begin slice | arena.
// The arena part is the leaves' byte range (or the leaves gathered back to back when scattered, as Stage).
struct MStage {
    size_t t0 = 0, t1 = 0, l0 = 0, l1 = 0, o_off = 0, o_len = 0, o_txb = 0, o_ar = 0, total = 0;
    uint64_t lo = 0, hi = 0;
    uint64_t extent = 0;   // as Stage::extent
    bool compact = false;
};
inline MStage mstage_plan(size_t t0, size_t t1, const uint32_t *txb, const uint64_t *off, const uint32_t *len,
                          WorkerPool *pool) {
    MStage st;
    st.t0 = t0;
    st.t1 = t1;
    st.l0 = txb[t0];
    st.l1 = txb[t1];
    const size_t nl = st.l1 - st.l0, nt = t1 - t0;
    const Span sp = nl ? arena_span(st.l0, st.l1, off, len, pool) : Span{0, 0, 0};
    const uint64_t lo = sp.lo & ~(uint64_t)15;
    st.compact = nl && sp.hi - lo > 2 * sp.bytes + (1u << 20);
    st.lo = st.compact ? 0 : (nl ? lo : 0);
    st.hi = st.compact ? sp.bytes : (nl ? sp.hi : 0);
    st.extent = nl ? sp.hi : 0;
    st.o_off = 0;
    st.o_len = al16(nl * 8);
    st.o_txb = st.o_len + al16(nl * 4);
    st.o_ar = st.o_txb + al16((nt + 1) * 4);
    st.total = st.o_ar + al16(st.hi - st.lo + 16);
    return st;
}
inline void mstage_pack(const MStage &st, uint8_t *h, const uint32_t *txb, const uint8_t *arena, const uint64_t *off,
                        const uint32_t *len, WorkerPool *pool) {
    const size_t nl = st.l1 - st.l0, nt = st.t1 - st.t0;
    uint64_t *hoff = reinterpret_cast<uint64_t *>(h + st.o_off);
    uint8_t *har = h + st.o_ar;
    if (st.compact) {
        par_copy({{h + st.o_len, len + st.l0, nl * 4}, {h + st.o_txb, txb + st.t0, (nt + 1) * 4}}, nullptr);
        uint64_t pos = 0;
        for (size_t i = 0; i < nl; i++) {
            hoff[i] = pos;
            if (len[st.l0 + i]) std::memcpy(har + pos, arena + off[st.l0 + i], len[st.l0 + i]);
            pos += len[st.l0 + i];
        }
    } else {
        par_copy({{h + st.o_off, off + st.l0, nl * 8}, {h + st.o_len, len + st.l0, nl * 4},
                  {h + st.o_txb, txb + st.t0, (nt + 1) * 4},
                  {har, st.hi > st.lo ? arena + st.lo : nullptr, (size_t)(st.hi - st.lo)}},
                 pool);
    }
    std::memset(har + (st.hi - st.lo), 0, 16);
}
inline bool mstage_direct(const MStage &st, const uint32_t *txb, const uint8_t *arena, const uint64_t *off,
                          const uint32_t *len) {
    if (st.compact) return false;
    const size_t nl = st.l1 - st.l0, nt = st.t1 - st.t0;
    return (nl == 0 || (host_pinned(off + st.l0, nl * 8) && host_pinned(len + st.l0, nl * 4))) &&
           host_pinned(txb + st.t0, (nt + 1) * 4) && (st.hi == st.lo || host_pinned(arena + st.lo, st.hi - st.lo));
}
inline hipError_t mstage_dma_direct(const MStage &st, uint8_t *dv, const uint32_t *txb, const uint8_t *arena,
                                    const uint64_t *off, const uint32_t *len, hipStream_t s) {
    const size_t nl = st.l1 - st.l0, nt = st.t1 - st.t0;
    hipError_t e = hipSuccess;
    if (nl) e = hipMemcpyAsync(dv + st.o_off, off + st.l0, nl * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && nl) e = hipMemcpyAsync(dv + st.o_len, len + st.l0, nl * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dv + st.o_txb, txb + st.t0, (nt + 1) * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && st.hi > st.lo)
        e = hipMemcpyAsync(dv + st.o_ar, arena + st.lo, st.hi - st.lo, hipMemcpyHostToDevice, s);
    return e;
}
// a Merkle stage's leaves inside the caller's arena (and none wrapping), checked before anything reads them
inline bool mstage_in_bounds(const MStage &st, uint64_t arena_bytes) {
    return st.extent != UINT64_MAX && st.extent <= arena_bytes;
}

// ---------------------------------------------------------------- key hash
// Key bytes come from untrusted submitters (and invalid keys are deduped before decoding), so the
// host hash tables hash all 32 bytes with a per-process random seed: a batch of keys that share some
// bytes cannot pile into one probe chain.  64-bit multiply-xorshift mixing of the four words, each
// folded with its own seed (a keyed hash in the wyhash / murmur-finaliser family: not cryptographic,
// only unpredictable to the submitter).
inline uint64_t key_seed(int k) {
    static const std::array<uint64_t, 5> seeds = [] {
        std::random_device rd;
        std::array<uint64_t, 5> s{};
        for (auto &x : s) x = ((uint64_t)rd() << 32) ^ rd() ^ (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
        return s;
    }();
    return seeds[k];
}
inline uint64_t mix64(uint64_t x) {
    x ^= x >> 32;
    x *= 0xd6e8feb86659fd93ull;
    x ^= x >> 32;
    x *= 0xd6e8feb86659fd93ull;
    x ^= x >> 32;
    return x;
}
inline uint64_t key_hash32(const uint8_t *k) {
    uint64_t w[4];
    std::memcpy(w, k, 32);
    uint64_t h = key_seed(4);
    for (int i = 0; i < 4; i++) h = mix64(h ^ (w[i] + key_seed(i)) * 0x9E3779B97F4A7C15ull) + (uint64_t)i;
    return h;
}

// ---------------------------------------------------------------- key dedupe
// Host-side key dedupe of the plain entry points: keys = the distinct key bytes in first-seen order,
// key_index[i] = its index.  Returns false when the batch does not repeat keys enough for the keyed path to
// pay (fewer than eight signatures per distinct key: a key's 66 KB of tables cost about 7 plain verifies).
//   - n > 4,096: a gate first samples s = 4 sqrt(n) signatures (512 .. 4,096) at pseudo-random positions (a fixed
//     sequence, so a batch always gets the same decision) and counts repeated keys among them; a batch of c
//     distinct keys shows about s^2 / 2c repeats in a sample of s, so fewer than 4 s^2 / 2n repeats (an
//     estimated ratio below four signatures per key) is taken as distinct-keyed without touching the rest.  A
//     performance guess only: both paths give the same verdicts.
//   - the dedupe proper runs in slices on the pool, each with its own growing open-addressing table (a
//     1,024-key pool stays in cache), giving up once any slice has seen more than n / 8 distinct keys;
//     the slices' key lists are then merged in slice order (first-seen order overall) and the slices'
//     local indices remapped.
// Flat tables on the seeded hash of all 32 key bytes (key_hash32), no per-key allocation.
struct FlatKeys {
    std::vector<uint32_t> first, id;   // bucket -> representative record, distinct-key index (UINT32_MAX = empty)
    size_t mask = 0, count = 0;
    explicit FlatKeys(size_t cap0 = 1024) { reset(cap0); }
    void reset(size_t cap) {
        size_t c = 64;
        while (c < cap) c <<= 1;
        first.assign(c, UINT32_MAX);
        id.assign(c, 0);
        mask = c - 1;
        count = 0;
    }
    // index of the key pk[32 * i] (inserting it as `fresh` when new); *added = whether it was new
    uint32_t find_or_add(const uint8_t *pk, uint32_t i, uint32_t fresh, bool *added) {
        const uint8_t *k = pk + 32 * (size_t)i;
        size_t bkt = (size_t)key_hash32(k) & mask;
        for (;;) {
            const uint32_t f = first[bkt];
            if (f == UINT32_MAX) {
                if (2 * (count + 1) > mask + 1) {   // grow: keep the load at or below 1/2
                    grow(pk);
                    return find_or_add(pk, i, fresh, added);
                }
                first[bkt] = i;
                id[bkt] = fresh;
                count++;
                *added = true;
                return fresh;
            }
            if (std::memcmp(pk + 32 * (size_t)f, k, 32) == 0) {
                *added = false;
                return id[bkt];
            }
            bkt = (bkt + 1) & mask;
        }
    }

  private:
    void grow(const uint8_t *pk) {
        std::vector<uint32_t> f0 = std::move(first), i0 = std::move(id);
        const size_t c = 2 * (mask + 1);
        first.assign(c, UINT32_MAX);
        id.assign(c, 0);
        mask = c - 1;
        for (size_t b = 0; b < f0.size(); b++) {
            if (f0[b] == UINT32_MAX) continue;
            size_t bkt = (size_t)key_hash32(pk + 32 * (size_t)f0[b]) & mask;
            while (first[bkt] != UINT32_MAX) bkt = (bkt + 1) & mask;
            first[bkt] = f0[b];
            id[bkt] = i0[b];
        }
    }
};

// The sample: s = 4 sqrt(n) records (512 .. 4,096): a batch with eight signatures per key then shows about
// 4 s^2 / n = 64 repeats, a distinct-keyed one about s^2 / (2 n) = 8, against a threshold of 2 s^2 / n = 32 —
// Poisson tails far below 10^-6 either way.  Round 4 sampled 4,096 records at every size above 16,384 and deduped
// every batch up to 16,384 in full: 60-100 us of host time on each distinct-keyed notary batch of 16,384-65,536
// signatures (tools/notary_probe.py host phases), for a decision that only picks the faster path.
// LSD radix sort of values below `bound` (passes of 11 bits up to bound's top bit): the gate's 4,096 sample
// positions, which std::sort took ~300 us to order on this container's host (radix: 60 us for three passes) —
// on every large call's path before its first DMA
inline void radix_sort_u32(std::vector<uint32_t> &v, uint64_t bound) {
    std::vector<uint32_t> tmp(v.size());
    for (int sh = 0; sh < 32 && (bound - 1) >> sh; sh += 11) {
        uint32_t cnt[2049] = {};
        for (uint32_t x : v) cnt[((x >> sh) & 2047) + 1]++;
        for (int k = 0; k < 2048; k++) cnt[k + 1] += cnt[k];
        for (uint32_t x : v) tmp[cnt[(x >> sh) & 2047]++] = x;
        v.swap(tmp);
    }
}

inline bool dedupe_gate(size_t n, const uint8_t *pk) {
    if (n <= 4096) return true;                    // the estimate needs s << n; a full dedupe of <= 4,096 is cheap
    const uint32_t kS = (uint32_t)std::min<double>(4096.0, std::max(512.0, 4.0 * std::sqrt((double)n)));
    FlatKeys t(4 * kS);                            // load <= 1/4: the table never grows while sampling
    uint64_t x = 0x9E3779B97F4A7C15ull;
    uint32_t rep = 0;
    std::vector<uint32_t> pos(kS);
    for (uint32_t j = 0; j < kS; j++) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        pos[j] = (uint32_t)((x >> 32) * (uint64_t)n >> 32);
    }
    radix_sort_u32(pos, n);                        // ascending: duplicate positions adjacent
    constexpr uint32_t kAhead = 16;                // the key reads miss the caches: prefetched 16 samples ahead
    for (uint32_t j = 0; j < std::min(kS, kAhead); j++) __builtin_prefetch(pk + 32 * (size_t)pos[j]);
    uint32_t prev = UINT32_MAX;
    for (uint32_t j = 0; j < kS; j++) {
        if (j + kAhead < kS) __builtin_prefetch(pk + 32 * (size_t)pos[j + kAhead]);
        if (pos[j] == prev) continue;               // the same record twice is not a repeated key
        prev = pos[j];
        bool added;
        t.find_or_add(pk, pos[j], (uint32_t)t.count, &added);
        rep += added ? 0 : 1;
    }
    // keyed worth a full dedupe when s^2 / (2 rep) < n / 4, i.e. rep > 2 s^2 / n
    return (double)rep > 2.0 * (double)kS * (double)kS / (double)n;
}

inline bool dedupe_keys(size_t n, const uint8_t *pk, std::vector<uint8_t> &keys, std::vector<uint32_t> &key_index,
                        WorkerPool *pool, bool gate = true) {
    if (n < 64 || n > 0xffffffffull) return false;
    if (gate && !dedupe_gate(n, pk)) return false;
    const size_t limit = n / 8;                      // most distinct keys the keyed path takes
    const int nt = pool ? pool->threads() : 1;
    const size_t nsl = (n >= 65536 && nt > 1) ? (size_t)nt * 2 : 1;
    const size_t per = (n + nsl - 1) / nsl;
    key_index.resize(n);
    std::vector<std::vector<uint32_t>> uniq(nsl);   // per slice: the record of each local key, first-seen order
    std::atomic<bool> over{false};
    auto slice = [&](size_t s) {
        const size_t b = s * per, e = std::min(n, b + per);
        FlatKeys t(1024);
        for (size_t i = b; i < e && !over.load(std::memory_order_relaxed); i++) {
            bool added;
            key_index[i] = t.find_or_add(pk, (uint32_t)i, (uint32_t)uniq[s].size(), &added);
            if (added) {
                uniq[s].push_back((uint32_t)i);
                if (uniq[s].size() > limit) over.store(true);
            }
        }
    };
    if (nsl > 1)
        pool->run(nsl, slice);
    else
        slice(0);
    if (over.load()) return false;
    // merge the slices' key lists in slice order; remap[s][local] = global index
    FlatKeys g(4096);
    std::vector<uint32_t> grec;                      // the representative record of each global key
    std::vector<std::vector<uint32_t>> remap(nsl);
    for (size_t s = 0; s < nsl; s++) {
        remap[s].resize(uniq[s].size());
        for (size_t u = 0; u < uniq[s].size(); u++) {
            bool added;
            remap[s][u] = g.find_or_add(pk, uniq[s][u], (uint32_t)grec.size(), &added);
            if (added) {
                grec.push_back(uniq[s][u]);
                if (grec.size() > limit) return false;
            }
        }
    }
    if (nsl > 1 || !remap[0].empty()) {
        auto fix = [&](size_t s) {
            const size_t b = s * per, e = std::min(n, b + per);
            const std::vector<uint32_t> &r = remap[s];
            for (size_t i = b; i < e; i++) key_index[i] = r[key_index[i]];
        };
        if (nsl > 1)
            pool->run(nsl, fix);
        else
            fix(0);
    }
    keys.resize(32 * grec.size());
    for (size_t u = 0; u < grec.size(); u++) std::memcpy(keys.data() + 32 * u, pk + 32 * (size_t)grec[u], 32);
    return true;
}

// ---------------------------------------------------------------- sub-chunk planners
// The pipeline's sub-chunk boundaries of [b, e): [first, C, C, ..., the last two balanced]; every boundary
// but e is b + a multiple of `align`.  With ramp, the sizes after the first double (first, 2 first, ...)
// until they reach C: each sub-chunk's copy then takes about as long as the kernels of the one before it,
// so the GPU is not left waiting for a big second sub-chunk while a small first one has long finished.
// The sub-chunk of an asynchronous pipelined call of n records: 1 or 2 x CV_OPT_ASYNC_CHUNK, the multiple nearest
// n / 16 (so a call has about 16 or fewer launch groups, each a whole number of async chunks).
inline size_t async_sub_chunk(size_t async_chunk, size_t n) {
    const size_t c = std::max<size_t>(64, async_chunk / 64 * 64);
    return c * std::min<size_t>(2, std::max<size_t>(1, (n / 16 + c / 2) / c));
}
inline std::vector<size_t> pipe_cuts(size_t b, size_t e, size_t first, size_t C, bool ramp = false, size_t align = 64) {
    std::vector<size_t> cut{b};
    if (e <= b) return cut;
    first = std::max<size_t>(align, first / align * align);
    C = std::max<size_t>(align, C / align * align);
    size_t p = b + std::min(e - b, first);
    cut.push_back(p);
    size_t step = first;
    while (p < e) {
        const size_t rem = e - p;
        step = ramp ? std::min(C, 2 * step) : C;
        const size_t m = rem <= step ? rem : rem < 2 * step ? (rem / 2 + align - 1) / align * align : step;
        p += m;
        cut.push_back(p);
    }
    return cut;
}
// The Merkle sub-chunk boundaries of transactions [t0, t1): whole transactions, each sub-chunk as many as keep its
// leaves (txb: ntx + 1 leaf boundaries) within its target, and at least one.  The target is `per` leaves; with ramp
// a quarter of it first (at least one leaf), then doubling up to `per`.  A target past the last 32-bit leaf index
// is clamped to it.
inline std::vector<size_t> merkle_cuts(const uint32_t *txb, size_t t0, size_t t1, size_t per, bool ramp) {
    std::vector<size_t> cut{t0};
    for (size_t want = ramp ? std::max<size_t>(1, per / 4) : per; cut.back() < t1; want = std::min(per, 2 * want)) {
        const size_t c = cut.back();
        const uint64_t target = (uint64_t)txb[c] + want;
        const size_t nx = (size_t)(std::upper_bound(txb + c + 1, txb + t1 + 1,
                                                    (uint32_t)std::min<uint64_t>(target, UINT32_MAX)) - txb) - 1;
        cut.push_back(std::min(std::max(nx, c + 1), t1));
    }
    return cut;
}

}  // namespace cvh
