// rl_cache.cpp — C-ABI implementation, part 4: the synchronous host-buffer calls
// (rl_optimize*, rl_lap_eval, rl_optimize_multi) and the plan cache behind them.
//
// rl_optimize and rl_lap_eval are the reference's own use: one synchronous call per track
// and mode (ref:1347, 1397, 1466-1478), host buffers in and out.  Building a plan per call
// (a hipMalloc per array, a stream, events) and copying through pageable memory cost more
// than the kernel at small B, so these calls reuse plans from a small process-wide cache,
// keyed by the plan's shape and the ring segments (compared bit for bit): a hit uploads
// only the centreline, cfg and seeds.  Every copy is staged through pinned host memory
// owned by the entry; results are downloaded array by array, each with an event, and
// host threads copy an array out as soon as its event completes.  An entry in use is
// checked out, so concurrent callers never share one.  The cache object is never
// destroyed (no HIP call at process exit); rl_release_plan_cache() frees the idle plans.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <mutex>
#include <thread>

#include <sys/mman.h>
#include <unistd.h>

#include "rl_host.h"

using namespace rl;

namespace {

constexpr int kCacheEntries = 8;                       // idle plans kept
// device + pinned host bytes kept idle (RL_PLAN_CACHE_MB overrides; 0 disables caching).
// An entry larger than the budget on its own is not kept either, so one oversized call
// leaves nothing allocated behind it.
constexpr size_t kCacheBytesDefault = (size_t)2 << 30;
size_t cache_budget() {
    const char* s = std::getenv("RL_PLAN_CACHE_MB");
    if (!s || !*s) return kCacheBytesDefault;
    char* end = nullptr;
    const unsigned long long mb = std::strtoull(s, &end, 10);
    if (end == s) return kCacheBytesDefault;
    return (size_t)mb << 20;
}
constexpr int kJobEvents = 512;   // download events of an entry (download_staged, download_overlapped)

struct CacheEntry {
    rl_plan* p = nullptr;
    int device = 0, N = 0, B = 0, ncfg = 0, mo = 0, closed = 0, Ei = 0, Eo = 0;
    bool stream = false, centers = false, Ls = false;
    std::vector<double> segs;                          // inner then outer segments
    unsigned char* pin = nullptr;                      // pinned staging
    size_t pin_bytes = 0;
    hipEvent_t ev[kJobEvents] = {};
    // overlapped download (download_overlapped): per-mode instance completion flags in
    // coherent pinned memory, the epoch of the last run, and the copy stream
    uint32_t* flags = nullptr;
    int flags_n = 0;
    uint32_t epoch = 0;
    hipStream_t dl = nullptr;
    uint64_t tick = 0;

    bool same(const CacheEntry& k) const {
        return device == k.device && N == k.N && B == k.B && ncfg == k.ncfg && mo == k.mo && closed == k.closed &&
               Ei == k.Ei && Eo == k.Eo && stream == k.stream && centers == k.centers && Ls == k.Ls &&
               segs.size() == k.segs.size() &&
               (segs.empty() || std::memcmp(segs.data(), k.segs.data(), segs.size() * sizeof(double)) == 0);
    }
    // device memory of the plan plus the pinned staging buffer (both stay allocated while idle)
    size_t bytes() const { return (p ? p->dev_bytes() : 0) + pin_bytes + (size_t)flags_n * sizeof(uint32_t); }
};

void destroy_entry(CacheEntry* e) {
    if (!e) return;
    if (e->p) {
        hipSetDevice(e->p->device);
        rl_plan_destroy(e->p);
    }
    for (hipEvent_t& v : e->ev)
        if (v) hipEventDestroy(v);
    if (e->dl) {
        hipStreamSynchronize(e->dl);
        hipStreamDestroy(e->dl);
    }
    if (e->flags) hipHostFree(e->flags);
    if (e->pin) hipHostFree(e->pin);
    delete e;
}

struct PlanCache {
    std::mutex mu;
    std::vector<CacheEntry*> idle;
    uint64_t tick = 0;

    CacheEntry* take(const CacheEntry& key) {
        std::lock_guard<std::mutex> g(mu);
        for (size_t i = 0; i < idle.size(); ++i)
            if (idle[i]->same(key)) {
                CacheEntry* e = idle[i];
                idle.erase(idle.begin() + (long)i);
                return e;
            }
        return nullptr;
    }
    void give(CacheEntry* e) {
        std::vector<CacheEntry*> evict;
        const size_t budget = cache_budget();
        {
            std::lock_guard<std::mutex> g(mu);
            e->tick = ++tick;
            idle.push_back(e);
            auto total = [&]() {
                size_t t = 0;
                for (CacheEntry* q : idle) t += q->bytes();
                return t;
            };
            // least recently used first, down to the newest entry itself when it alone
            // exceeds the budget
            while (!idle.empty() && ((int)idle.size() > kCacheEntries || total() > budget)) {
                auto lru = std::min_element(idle.begin(), idle.end(),
                                            [](CacheEntry* x, CacheEntry* y) { return x->tick < y->tick; });
                evict.push_back(*lru);
                idle.erase(lru);
            }
        }
        for (CacheEntry* q : evict) destroy_entry(q);
    }
    void info(int32_t* entries, int64_t* dev_bytes, int64_t* pin_bytes) {
        std::lock_guard<std::mutex> g(mu);
        int64_t d = 0, h = 0;
        for (CacheEntry* q : idle) {
            d += q->p ? (int64_t)q->p->dev_bytes() : 0;
            h += (int64_t)q->pin_bytes;
        }
        if (entries) *entries = (int32_t)idle.size();
        if (dev_bytes) *dev_bytes = d;
        if (pin_bytes) *pin_bytes = h;
    }
    void clear() {
        std::vector<CacheEntry*> all;
        {
            std::lock_guard<std::mutex> g(mu);
            all.swap(idle);
        }
        for (CacheEntry* q : all) destroy_entry(q);
    }
};
PlanCache& plan_cache() {
    static PlanCache* c = new PlanCache();
    return *c;
}

thread_local float g_last_kernel_ms = -1.0f, g_last_call_ms = -1.0f;
thread_local float g_last_mode_ms[2] = {-1.0f, -1.0f};    // min-curv / min-time kernel of the last call
thread_local int g_last_groups = 0, g_last_groups_signalled = 0;   // the last call's download groups

int ensure_pinned(CacheEntry* e, size_t bytes) {
    if (bytes <= e->pin_bytes) return RL_OK;
    if (e->pin) hipHostFree(e->pin);
    e->pin = nullptr;
    e->pin_bytes = 0;
    const size_t want = std::max(bytes, (size_t)1 << 16);
    if (hipHostMalloc((void**)&e->pin, want, hipHostMallocDefault) != hipSuccess) {
        e->pin = nullptr;
        return fail(RL_ENOMEM, "hipHostMalloc (pinned staging) failed");
    }
    e->pin_bytes = want;
    return RL_OK;
}

// Download `jobs` through the entry's pinned staging (from byte `base` on): one async copy
// per job on stream st with an event after each (the last event covers any jobs beyond
// the pool), then host threads copy each job out in 4 MiB pieces as soon as its event has
// completed, so the host copies overlap the transfers still in flight.
int download_staged(CacheEntry* e, hipStream_t st, const std::vector<CopyJob>& jobs, size_t base) {
    struct Piece {
        unsigned char* dst;
        const unsigned char* src;
        size_t bytes;
        int ev;
    };
    std::vector<Piece> pieces;
    size_t off = base, total = 0;
    const size_t kPiece = (size_t)4 << 20;
    for (size_t j = 0; j < jobs.size(); ++j) {
        if (hipMemcpyAsync(e->pin + off, jobs[j].src, jobs[j].bytes, hipMemcpyDeviceToHost, st) != hipSuccess)
            return fail(RL_EHIP, "download (staged) failed");
        const int evi = (int)std::min(j, (size_t)kJobEvents - 1);
        const bool last = j + 1 == jobs.size();
        if ((size_t)evi == j || last)
            if (hipEventRecord(e->ev[evi], st) != hipSuccess) return fail(RL_EHIP, "hipEventRecord failed");
        for (size_t q = 0; q < jobs[j].bytes; q += kPiece)
            pieces.push_back({(unsigned char*)jobs[j].dst + q, e->pin + off + q, std::min(kPiece, jobs[j].bytes - q), evi});
        off += (jobs[j].bytes + 255) & ~(size_t)255;
        total += jobs[j].bytes;
    }
    std::atomic<size_t> next{0};
    std::atomic<bool> bad{false};
    auto work = [&]() {
        for (size_t i; (i = next.fetch_add(1)) < pieces.size();) {
            if (hipEventSynchronize(e->ev[pieces[i].ev]) != hipSuccess) {
                bad = true;
                return;
            }
            std::memcpy(pieces[i].dst, pieces[i].src, pieces[i].bytes);
        }
    };
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int nthr = total < ((size_t)8 << 20) ? 1 : (int)std::min<size_t>({8, hw, pieces.size()});
    // helper threads are an optimisation: if one cannot be started (std::system_error,
    // std::bad_alloc), the calling thread does its share, and no exception leaves the C ABI
    std::vector<std::thread> th;
    try {
        th.reserve((size_t)std::max(0, nthr - 1));
        for (int t = 1; t < nthr; ++t) th.emplace_back(work);
    } catch (...) {
    }
    work();
    for (auto& t : th) t.join();
    if (bad) return fail(RL_EHIP, "download (staged): event wait failed");
    return RL_OK;
}

// bytes of the staging area a job list needs (256-B aligned pieces)
size_t staged_bytes(const std::vector<CopyJob>& jobs) {
    size_t t = 0;
    for (const CopyJob& j : jobs) t += (j.bytes + 255) & ~(size_t)255;
    return t;
}

// ---- overlapped download (large batches)
// The kernel of an rl_optimize call finishes its instances over its whole run (a batch of
// B instances takes B / (instances resident) rounds), but a download that waits for the
// kernel moves all of their results after it (C2: 98 MB, 40 % of the call).
// Here every instance signals its completion (KParams::done, signal_done in rl_kernels.h)
// into coherent pinned memory; the calling thread watches the flags and, as soon as every
// instance of a group has signalled, queues that group's result slices (instance-major
// arrays: one contiguous slice per array) on a copy stream, while the kernel still computes
// later instances.  Helper threads copy each group out of the pinned staging as its copies
// land.  The launch is the one rl_plan_run makes anyway, so the results are those of the
// plan path bit for bit.  A kernel that ends without signalling some instance (or any HIP
// failure) takes the stream-ordered path for the rest: the copy stream waits for the
// kernel's end event.  RL_OVERLAP_DOWNLOAD=0 turns the overlap off (A/B, tests).
constexpr size_t kOverlapMinBytes = (size_t)8 << 20;  // smaller downloads: one staged pass
constexpr int kGroupsPerMode = 16;                     // groups of a mode
static_assert(2 * kGroupsPerMode <= kJobEvents, "one download event per group");

bool overlap_enabled() {
    const char* s = std::getenv("RL_OVERLAP_DOWNLOAD");
    return !(s && s[0] == '0');
}

int ensure_flags(CacheEntry* e, int B) {
    if (!e->dl && hipStreamCreateWithFlags(&e->dl, hipStreamNonBlocking) != hipSuccess) {
        e->dl = nullptr;
        return fail(RL_EHIP, "hipStreamCreate (download stream) failed");
    }
    if (e->flags && e->flags_n >= 2 * B) return RL_OK;
    if (e->flags) hipHostFree(e->flags);
    e->flags = nullptr;
    e->flags_n = 0;
    if (hipHostMalloc((void**)&e->flags, (size_t)2 * B * sizeof(uint32_t), hipHostMallocCoherent | hipHostMallocMapped) !=
        hipSuccess) {
        e->flags = nullptr;
        return fail(RL_ENOMEM, "hipHostMalloc (completion flags) failed");
    }
    std::memset(e->flags, 0, (size_t)2 * B * sizeof(uint32_t));
    e->flags_n = 2 * B;
    e->epoch = 0;
    return RL_OK;
}

// Ask the kernel for writable pages behind [p, p + n) now (MADV_POPULATE_WRITE, Linux 5.14;
// errors ignored): a page already present is left as it is, so this never changes the
// caller's data and may run while another thread copies into the same range.  Fresh output
// arrays (the reference's own use) would otherwise take their page faults inside the copies
// after the kernel.
void populate_write(void* p, size_t n) {
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif
    static const uintptr_t pg = (uintptr_t)sysconf(_SC_PAGESIZE);
    if (!n) return;
    const uintptr_t a = (uintptr_t)p & ~(pg - 1), b = ((uintptr_t)p + n + pg - 1) & ~(pg - 1);
    (void)madvise((void*)a, b - a, MADV_POPULATE_WRITE);
}

#ifdef RL_OVL_TRACE
// diagnostic builds: times (ms since the call's entry) of one rl_optimize call, printed to
// stderr as one JSON line when the call returns
struct OvlTrace {
    std::chrono::steady_clock::time_point t0;
    double launched = -1, kend = -1, dma = -1, copied = -1;
    int nthr = 0;
    std::vector<double> pub;
};
thread_local OvlTrace g_tr;
double tr_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g_tr.t0).count(); }
#endif

// jm[m]: mode m's download jobs (out_jobs order, every array instance-major over the plan's B
// instances).  Called after rl_plan_run queued the kernels with p->done set.
int download_overlapped(CacheEntry* e, rl_plan* p, const std::vector<CopyJob> (&jm)[2], uint32_t epoch) {
    const int B = p->B;
    const int G = std::min(kGroupsPerMode, B);
    struct Group {
        int m, b0, b1;
        int s0, s1;                                    // its slices [s0, s1)
    };
    struct Piece {
        unsigned char* dst;
        const unsigned char* src;
        size_t bytes;
        int slice;
    };
    std::vector<Group> groups;
    for (int m = 0; m < 2; ++m)
        if (!jm[m].empty())
            for (int g = 0; g < G; ++g)
                groups.push_back({m, (int)((int64_t)B * g / G), (int)((int64_t)B * (g + 1) / G), 0, 0});
    // staging offsets: array-major, as download_staged lays them out
    std::vector<size_t> job_off[2];
    size_t off = 0;
    for (int m = 0; m < 2; ++m)
        for (const CopyJob& j : jm[m]) {
            job_off[m].push_back(off);
            off += (j.bytes + 255) & ~(size_t)255;
        }
    // slices in publication order (group-major): slice g.s0 + k is array k of group g;
    // slice_ev[s] is the event recorded after its copy (set when queued, before publication)
    std::vector<int> slice_ev;
    std::vector<Piece> pieces;
    const size_t kPiece = (size_t)1 << 20;
    for (Group& g : groups) {
        g.s0 = (int)slice_ev.size();
        for (size_t k = 0; k < jm[g.m].size(); ++k) {
            const CopyJob& j = jm[g.m][k];
            const size_t row = j.bytes / (size_t)B;    // bytes of one instance
            const size_t o = (size_t)g.b0 * row, n = (size_t)(g.b1 - g.b0) * row;
            const int si = (int)slice_ev.size();
            slice_ev.push_back(-1);
            for (size_t q = 0; q < n; q += kPiece)
                pieces.push_back({(unsigned char*)j.dst + o + q, e->pin + job_off[g.m][k] + o + q, std::min(kPiece, n - q), si});
        }
        g.s1 = (int)slice_ev.size();
    }
    std::atomic<size_t> next{0}, next_pop{0};
    std::atomic<int> published{0};                     // slices queued (publication order)
    std::atomic<bool> bad{false};
    auto work = [&](bool populate) {
        if (populate)                                  // while the first instances still compute
            for (size_t i; (i = next_pop.fetch_add(1)) < jm[0].size() + jm[1].size();) {
                const CopyJob& j = i < jm[0].size() ? jm[0][i] : jm[1][i - jm[0].size()];
                populate_write(j.dst, j.bytes);
            }
        for (size_t i; (i = next.fetch_add(1)) < pieces.size();) {
            const int si = pieces[i].slice;
            while (published.load(std::memory_order_acquire) <= si) {
                if (bad.load()) return;
                std::this_thread::sleep_for(std::chrono::microseconds(10));
            }
            if (hipEventSynchronize(e->ev[slice_ev[si]]) != hipSuccess) {
                bad = true;
                return;
            }
            std::memcpy(pieces[i].dst, pieces[i].src, pieces[i].bytes);
        }
    };
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int nthr = (int)std::min<size_t>({8, hw, pieces.size() + 1});
    std::vector<std::thread> th;
    try {
        th.reserve((size_t)std::max(0, nthr - 1));
        for (int t = 1; t < nthr; ++t) th.emplace_back(work, true);
    } catch (...) {
    }
    // the calling thread watches the flags and queues each finished group's copies
    const volatile uint32_t* fl = e->flags;
    bool joined[2] = {false, false};
    int signalled = 0;
#ifdef RL_OVL_TRACE     // diagnostic builds: when each group was queued, and the kernel's end
    g_tr.pub.assign(groups.size(), -1.0);
#endif
    auto group_done = [&](const Group& g) {
        for (int b = g.b0; b < g.b1; ++b)
            if (fl[(size_t)g.m * B + b] != epoch) return false;
        return true;
    };
    int next_ev = 0;
    for (size_t gi = 0; gi < groups.size() && !bad.load();) {
        const Group& g = groups[gi];
        for (int b = g.b0;;) {
            while (b < g.b1 && fl[(size_t)g.m * B + b] == epoch) ++b;
            if (b == g.b1) break;
            if (joined[g.m]) break;
            const hipError_t q = hipEventQuery(p->ev_end[g.m]);
            if (q == hipSuccess) {
                // the kernel has ended: every flag it stored is visible now, so a flag that
                // arrived between the read above and the query counts as signalled
                while (b < g.b1 && fl[(size_t)g.m * B + b] == epoch) ++b;
                if (b == g.b1) break;
                // ended without this flag: stream order from here on
                if (hipStreamWaitEvent(e->dl, p->ev_end[g.m], 0) != hipSuccess) bad = true;
                joined[g.m] = true;
                break;
            }
            if (q != hipErrorNotReady) {
                bad = true;
                break;
            }
            std::this_thread::yield();
        }
        if (bad.load()) break;
        // the batch: this group and every following group of the mode that is complete too
        // (after the kernel's end, all of them) -- one copy per array over the batch, so a
        // burst of finishing instances moves as few large copies (1 MB copies ran at ~21 GB/s,
        // against 56 GB/s for large ones: round-6 trace)
        size_t ge = gi + 1;
        while (ge < groups.size() && groups[ge].m == g.m && (joined[g.m] || group_done(groups[ge]))) ++ge;
        const Group& gl = groups[ge - 1];
        for (size_t k = 0; k < jm[g.m].size() && !bad.load(); ++k) {
            const CopyJob& j = jm[g.m][k];
            const size_t row = j.bytes / (size_t)B;
            const size_t o = (size_t)g.b0 * row, n = (size_t)(gl.b1 - g.b0) * row;
            const int ev = std::min(next_ev++, kJobEvents - 1);   // (a reused event only waits longer)
            if (hipMemcpyAsync(e->pin + job_off[g.m][k] + o, (const unsigned char*)j.src + o, n, hipMemcpyDeviceToHost,
                               e->dl) != hipSuccess ||
                hipEventRecord(e->ev[ev], e->dl) != hipSuccess)
                bad = true;
            for (size_t h = gi; h < ge; ++h) slice_ev[groups[h].s0 + k] = ev;
        }
        if (bad.load()) break;
        published.store(gl.s1, std::memory_order_release);
        for (size_t h = gi; h < ge; ++h) {
            if (!joined[g.m]) ++signalled;
#ifdef RL_OVL_TRACE
            g_tr.pub[h] = tr_ms();
#endif
        }
        gi = ge;
    }
#ifdef RL_OVL_TRACE
    if (hipEventSynchronize(p->ev_end[groups.back().m]) == hipSuccess) g_tr.kend = tr_ms();
    if (!slice_ev.empty() && slice_ev.back() >= 0 && hipEventSynchronize(e->ev[slice_ev.back()]) == hipSuccess)
        g_tr.dma = tr_ms();
    g_tr.nthr = nthr;
#endif
    work(false);
    for (auto& t : th) t.join();
#ifdef RL_OVL_TRACE
    g_tr.copied = tr_ms();
#endif
    const bool synced = hipStreamSynchronize(e->dl) == hipSuccess;
    if (bad.load() || !synced) return fail(RL_EHIP, "download (overlapped) failed");
    g_last_groups = (int)groups.size();
    g_last_groups_signalled = signalled;
    return RL_OK;
}

// rl_optimize_best's part of a cached call: select after the run and download only the winners
struct BestArgs {
    const rl_select* sel;
    int32_t* index;
    double* score;
    double* all_scores;
    rl_out* out;
    int32_t score_kind;               // RL_SCORE_DEFAULT or RL_SCORE_LAP
    // rl_optimize_best_trajectory: the winners' trajectories too (traj nullptr: none)
    double traj_dt = 0.0;
    int32_t traj_M = 0;
    rl_traj* traj = nullptr;
};

// rl_optimize / rl_lap_eval through the plan cache (see above), on the calling thread's
// current device.  kms[0..2]: HIP-event times of the whole run, the min-curvature and the
// min-time kernel (-1 if not run).
// best (rl_optimize_best, arguments already checked): no full download (out_mc / out_mt are
// NULL, so no download jobs, no completion flags, no overlapped path); the selection stage
// follows the run on the same stream and its G*k rows come back in one staged pass.
int run_cached(const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg, const uint64_t* seeds, int32_t B,
               int32_t modes, const double* centers, const double* Ls, rl_out* out_mc, rl_out* out_mt, float* kms,
               const BestArgs* best = nullptr) {
    const auto t0 = std::chrono::steady_clock::now();
#ifdef RL_OVL_TRACE
    g_tr = OvlTrace{};
    g_tr.t0 = t0;
#endif
    g_last_kernel_ms = g_last_call_ms = g_last_mode_ms[0] = g_last_mode_ms[1] = -1.0f;
    g_last_groups = g_last_groups_signalled = 0;
    if (int rc = check_inputs(prob, cfg, n_cfg, B, modes, centers)) return rc;
    const int ndev = rl_device_count();
    int dev = 0;
    if (ndev <= 0) return fail(RL_ENODEV, "no HIP device");
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= ndev) dev = 0;
    CacheEntry key;
    key.device = dev;
    key.N = prob->N;
    key.B = B;
    key.ncfg = n_cfg;
    key.mo = cfg[0].max_outer_iters;
    key.closed = prob->closed ? 1 : 0;
    key.Ei = prob->Ei;
    key.Eo = prob->Eo;
    key.stream = use_stream(prob->N);
    key.centers = centers != nullptr;
    key.Ls = Ls != nullptr;
    key.segs.assign(prob->inner_seg, prob->inner_seg + 4 * (size_t)prob->Ei);
    key.segs.insert(key.segs.end(), prob->outer_seg, prob->outer_seg + 4 * (size_t)prob->Eo);
    PlanCache& pc = plan_cache();
    CacheEntry* e = pc.take(key);
    const size_t N2 = 2 * (size_t)std::max(prob->N, 1);
    const size_t up_ctr = prob->N > 0 ? (centers ? (size_t)B : 1) * N2 * sizeof(double) : 0;
    const size_t up_ls = Ls ? (size_t)B * sizeof(double) : 0;
    const size_t up_cfg = (size_t)n_cfg * sizeof(rl_cfg), up_seed = (size_t)B * sizeof(uint64_t);
    const size_t up_bytes = ((up_ctr + 255) & ~(size_t)255) + ((up_ls + 255) & ~(size_t)255) +
                            ((up_cfg + 255) & ~(size_t)255) + up_seed;
    int rc = RL_OK;
    auto drop = [&](int code) {
        const std::string msg = g_err;
        destroy_entry(e);
        g_err = msg;
        return code;
    };
    if (!e) {
        rl_plan* p = nullptr;
        if ((rc = plan_create_ex(&p, dev, prob, cfg, n_cfg, seeds, B, modes, centers, Ls))) return rc;
        e = new CacheEntry(std::move(key));
        e->p = p;
        for (hipEvent_t& v : e->ev)
            if (hipEventCreateWithFlags(&v, hipEventDisableTiming) != hipSuccess) return drop(fail(RL_EHIP, "hipEventCreate failed"));
    } else {
        rl_plan* p = e->p;
        if (hipSetDevice(p->device) != hipSuccess) return drop(fail(RL_EHIP, "hipSetDevice failed"));
        for (int m = 0; m < 2; ++m)
            if ((modes & (1 << m)) && (rc = alloc_mode(p, m))) return drop(rc);
        p->L = prob->L;
        p->veh_width = prob->veh_width;
        if ((rc = ensure_pinned(e, up_bytes))) return drop(rc);
        hipStream_t st = p->own_stream;
        size_t off = 0;
        auto up = [&](void* d, const void* h, size_t bytes) -> bool {
            if (!bytes) return true;
            std::memcpy(e->pin + off, h, bytes);
            const bool ok = hipMemcpyAsync(d, e->pin + off, bytes, hipMemcpyHostToDevice, st) == hipSuccess;
            off += (bytes + 255) & ~(size_t)255;
            return ok;
        };
        std::vector<uint64_t> sd;
        if (!seeds) sd.assign((size_t)B, 0);
        if (!up(p->d_center, centers ? centers : prob->center_xy, up_ctr) || !up(p->d_Ls, Ls, up_ls) ||
            !up(p->d_cfg, cfg, up_cfg) || !up(p->d_seeds, seeds ? seeds : sd.data(), up_seed))
            return drop(fail(RL_EHIP, "upload (staged) failed"));
        set_margin(p, cfg, n_cfg);
    }
    rl_plan* p = e->p;
    p->modes = modes;
    std::vector<CopyJob> jm[2], jobs;
    out_jobs(p, 0, (modes & RL_MODE_MINCURV) ? out_mc : nullptr, jm[0]);
    out_jobs(p, 1, (modes & RL_MODE_MINTIME) ? out_mt : nullptr, jm[1]);
    jobs = jm[0];
    jobs.insert(jobs.end(), jm[1].begin(), jm[1].end());
    // the staging area serves the uploads first, then (after the kernel has started, or
    // stream-ordered after it) the downloads; a reallocation waits for the uploads queued
    size_t down_bytes = staged_bytes(jobs);
    if (best) {
        // the selection's jobs exist only after rl_plan_select: an upper bound of their staging
        // (16 jobs at most, each rounded up to 256 B), so the buffer is in place before the run
        const size_t gs = best->sel->group_size ? (size_t)best->sel->group_size : (size_t)B;
        const size_t R = (size_t)B / gs * (size_t)best->sel->k, mo = (size_t)p->max_outer;
        down_bytes = 16 * 256 + R * (8 * (size_t)p->N * 8 + 8 + (3 * mo + 1) * 4 + 12) + (size_t)B * 8;
        // and of the trajectory's jobs: 7 columns, the stamps, T and count
        if (best->traj)
            down_bytes += 10 * 256 + R * (((size_t)TRAJ_COLS * (size_t)best->traj_M + (size_t)p->N + 2) * 8 + 4);
    }
    if (down_bytes > e->pin_bytes) {
        if (hipStreamSynchronize(p->own_stream) != hipSuccess) return drop(fail(RL_EHIP, "upload sync"));
        if ((rc = ensure_pinned(e, down_bytes))) return drop(rc);
    }
    const bool overlap = !best && overlap_enabled() && p->N > 0 && B >= 2 && down_bytes >= kOverlapMinBytes;
    uint32_t epoch = 0;
    if (overlap) {
        if ((rc = ensure_flags(e, B))) return drop(rc);
        uint32_t* dflags = nullptr;
        if (hipHostGetDevicePointer((void**)&dflags, e->flags, 0) != hipSuccess || !dflags)
            return drop(fail(RL_EHIP, "hipHostGetDevicePointer (completion flags) failed"));
        if (++e->epoch == 0) {                         // wrapped: no flag may hold the new epoch
            std::memset(e->flags, 0, (size_t)e->flags_n * sizeof(uint32_t));
            e->epoch = 1;
        }
        epoch = e->epoch;
        p->epoch = epoch;
        // (test hook RL_OVERLAP_TEST_NOSIGNAL=1: the kernels do not signal, so every group takes
        // the stream-ordered fallback after the kernel's end -- tests/test_gpu_parity.py)
        const char* ns = std::getenv("RL_OVERLAP_TEST_NOSIGNAL");
        const bool nosig = ns && ns[0] == '1';
        for (int m = 0; m < 2; ++m) p->done[m] = (jm[m].empty() || nosig) ? nullptr : dflags + (size_t)m * B;
    }
    rc = rl_plan_run(p, nullptr);
#ifdef RL_OVL_TRACE
    g_tr.launched = tr_ms();
#endif
    p->done[0] = p->done[1] = nullptr;                 // later runs of this plan signal nothing
    if (rc) return drop(rc);
    if (best) {
        if ((rc = rl_plan_select_scored(p, best->sel, best->score_kind, nullptr))) return drop(rc);
        if (best->traj && (rc = rl_plan_trajectory(p, best->sel->mode, RL_TRAJ_SELECTED, best->traj_dt, best->traj_M, nullptr)))
            return drop(rc);
        jobs.clear();
        sel_jobs(p, best->index, best->score, best->all_scores, best->out, jobs);
        if (best->traj) traj_jobs(p, best->traj, jobs);
        if (staged_bytes(jobs) > e->pin_bytes) return drop(fail(RL_EHIP, "selection staging larger than its bound"));
        rc = download_staged(e, p->own_stream, jobs, 0);
    } else if (overlap) rc = download_overlapped(e, p, jm, epoch);
    else rc = download_staged(e, p->own_stream, jobs, 0);
    if (rc) return drop(rc);
    if (hipStreamSynchronize(p->own_stream) != hipSuccess) return drop(fail(RL_EHIP, "stream sync"));
    float ms[3] = {-1.0f, -1.0f, -1.0f};
    for (int i = 0; i < 3; ++i) {
        const bool has = i == 0 || (i == 1 && (modes & RL_MODE_MINCURV)) || (i == 2 && (modes & RL_MODE_MINTIME));
        if (has && (rc = rl_plan_kernel_ms(p, i, &ms[i]))) return drop(rc);
    }
    if (kms) std::memcpy(kms, ms, sizeof(ms));
    pc.give(e);
    g_last_kernel_ms = ms[0];
    g_last_mode_ms[0] = ms[1];
    g_last_mode_ms[1] = ms[2];
    g_last_call_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
#ifdef RL_OVL_TRACE
    std::fprintf(stderr, "{\"ovl_trace\": {\"launched_ms\": %.3f, \"kernel_ms\": %.3f, \"kernel_end_seen_ms\": %.3f, "
                 "\"dma_done_ms\": %.3f, \"copies_done_ms\": %.3f, \"return_ms\": %.3f, \"threads\": %d, \"published_ms\": [",
                 g_tr.launched, ms[1] > 0 ? ms[1] : ms[2], g_tr.kend, g_tr.dma, g_tr.copied, tr_ms(), g_tr.nthr);
    for (size_t i = 0; i < g_tr.pub.size(); ++i) std::fprintf(stderr, "%s%.3f", i ? ", " : "", g_tr.pub[i]);
    std::fprintf(stderr, "]}}\n");
#endif
    return RL_OK;
}

}  // namespace

extern "C" {

int rl_optimize(const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg, const uint64_t* seeds, int32_t B,
                rl_out* out_mincurv, rl_out* out_mintime) {
    int modes = (out_mincurv ? RL_MODE_MINCURV : 0) | (out_mintime ? RL_MODE_MINTIME : 0);
    if (!modes) return fail(RL_EINVAL, "no output requested");
    return run_cached(prob, cfg, n_cfg, seeds, B, modes, nullptr, nullptr, out_mincurv, out_mintime, nullptr);
}

int rl_optimize_best_scored(const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg, const uint64_t* seeds, int32_t B,
                            const rl_select* sel, int32_t score, int32_t* index, double* score_out,
                            double* all_scores, rl_out* out) {
    if (!sel || !index || !score_out) return fail(RL_EINVAL, "rl_optimize_best: sel / index / score is NULL");
    if (score != RL_SCORE_DEFAULT && score != RL_SCORE_LAP) return fail(RL_EINVAL, "select: unknown score");
    if (sel->mode != RL_MODE_MINCURV && sel->mode != RL_MODE_MINTIME)
        return fail(RL_EINVAL, "select: mode must be exactly one of RL_MODE_MINCURV, RL_MODE_MINTIME");
    if (int rc = check_inputs(prob, cfg, n_cfg, B, sel->mode, nullptr)) return rc;
    int gs = 0;
    if (int rc = check_select(sel, B, prob->N, sel->mode, &gs)) return rc;
    const BestArgs best{sel, index, score_out, all_scores, out, score};
    return run_cached(prob, cfg, n_cfg, seeds, B, sel->mode, nullptr, nullptr, nullptr, nullptr, nullptr, &best);
}

int rl_optimize_best_trajectory(const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg, const uint64_t* seeds, int32_t B,
                                const rl_select* sel, int32_t score, int32_t* index, double* score_out,
                                double* all_scores, rl_out* out, double dt, int32_t M_cap, rl_traj* traj) {
    if (!sel || !index || !score_out || !traj) return fail(RL_EINVAL, "rl_optimize_best_trajectory: sel / index / score / traj is NULL");
    if (score != RL_SCORE_DEFAULT && score != RL_SCORE_LAP) return fail(RL_EINVAL, "select: unknown score");
    if (sel->mode != RL_MODE_MINCURV && sel->mode != RL_MODE_MINTIME)
        return fail(RL_EINVAL, "select: mode must be exactly one of RL_MODE_MINCURV, RL_MODE_MINTIME");
    if (int rc = check_traj(dt, M_cap)) return rc;
    if (int rc = check_inputs(prob, cfg, n_cfg, B, sel->mode, nullptr)) return rc;
    int gs = 0;
    if (int rc = check_select(sel, B, prob->N, sel->mode, &gs)) return rc;
    BestArgs best{sel, index, score_out, all_scores, out, score};
    best.traj_dt = dt;
    best.traj_M = M_cap;
    best.traj = traj;
    return run_cached(prob, cfg, n_cfg, seeds, B, sel->mode, nullptr, nullptr, nullptr, nullptr, nullptr, &best);
}

int rl_optimize_best(const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg, const uint64_t* seeds, int32_t B,
                     const rl_select* sel, int32_t* index, double* score, double* all_scores, rl_out* out) {
    return rl_optimize_best_scored(prob, cfg, n_cfg, seeds, B, sel, RL_SCORE_DEFAULT, index, score, all_scores, out);
}

// B lap evaluations: heading_curv_from_points_generic + velocity_profile_forward_backward
// with h = L[b]/N on path b (ref:1045-1048, and the debug laps ref:1466-1478) = the
// min-time driver with max_outer_iters = 0 on per-instance centres.
int rl_lap_eval(const double* paths_xy, const double* L, int32_t N, int32_t B, int32_t closed, const rl_cfg* cfg,
                int32_t n_cfg, int32_t device, rl_out* out, float* kernel_ms) {
    if (!paths_xy || !L || !cfg || !out) return fail(RL_EINVAL, "rl_lap_eval: NULL argument");
    if (B < 1 || N < 0) return fail(RL_EINVAL, "rl_lap_eval: B < 1 or N < 0");
    if (n_cfg != 1 && n_cfg != B) return fail(RL_EINVAL, "n_cfg must be 1 or B");
    std::vector<rl_cfg> c(cfg, cfg + n_cfg);
    for (auto& x : c) x.max_outer_iters = 0;
    rl_problem pr{};
    pr.N = N;
    pr.closed = closed;
    pr.L = L[0];
    int cur = 0;
    const bool restore = hipGetDevice(&cur) == hipSuccess;
    if (int rc = select_device(device)) return rc;
    float ms[3];
    const int rc = run_cached(&pr, c.data(), n_cfg, nullptr, B, RL_MODE_MINTIME, paths_xy, L, nullptr, out, ms);
    if (rc == RL_OK && kernel_ms) *kernel_ms = ms[2];
    if (restore) hipSetDevice(cur);
    return rc;
}

int rl_last_call_ms(float* kernel_ms, float* call_ms) {
    if (g_last_call_ms < 0.0f) return fail(RL_EINVAL, "no successful rl_optimize / rl_lap_eval on this thread");
    if (kernel_ms) *kernel_ms = g_last_kernel_ms;
    if (call_ms) *call_ms = g_last_call_ms;
    return RL_OK;
}

int rl_last_call_times(float* run_ms, float* mincurv_ms, float* mintime_ms, float* call_ms) {
    if (g_last_call_ms < 0.0f) return fail(RL_EINVAL, "no successful rl_optimize / rl_lap_eval on this thread");
    if (run_ms) *run_ms = g_last_kernel_ms;
    if (mincurv_ms) *mincurv_ms = g_last_mode_ms[0];
    if (mintime_ms) *mintime_ms = g_last_mode_ms[1];
    if (call_ms) *call_ms = g_last_call_ms;
    return RL_OK;
}

int rl_last_call_download(int32_t* groups, int32_t* groups_signalled) {
    if (g_last_call_ms < 0.0f) return fail(RL_EINVAL, "no successful rl_optimize / rl_lap_eval on this thread");
    if (groups) *groups = g_last_groups;
    if (groups_signalled) *groups_signalled = g_last_groups_signalled;
    return RL_OK;
}

int rl_plan_cache_info(int32_t* entries, int64_t* device_bytes, int64_t* pinned_bytes) {
    plan_cache().info(entries, device_bytes, pinned_bytes);
    return RL_OK;
}

int rl_release_plan_cache(void) {
    int dev = 0;
    const bool have = hipGetDevice(&dev) == hipSuccess;
    plan_cache().clear();
    if (have) hipSetDevice(dev);
    return RL_OK;
}

// rl_optimize over several devices (SURVEY §8b device list, §8e): contiguous instance
// blocks, one plan and stream per device, every device enqueued before the first
// download, and each block's results copied to its offset of the caller's host outputs
// (the final gather).  Instances never span devices: block d holds [b0_d, b1_d).
int rl_optimize_multi(const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg, const uint64_t* seeds, int32_t B,
                      const int32_t* devices, int32_t n_dev, rl_out* out_mincurv, rl_out* out_mintime) {
    int modes = (out_mincurv ? RL_MODE_MINCURV : 0) | (out_mintime ? RL_MODE_MINTIME : 0);
    if (!modes) return fail(RL_EINVAL, "no output requested");
    if (n_dev < 1) return fail(RL_EINVAL, "n_dev must be >= 1");
    // every cfg (all blocks) is checked up front: the output offsets below use cfg[0]'s
    // max_outer_iters for every block
    if (int rc0 = check_inputs(prob, cfg, n_cfg, B, modes, nullptr)) return rc0;
    const int ndev = rl_device_count();
    if (ndev <= 0) return fail(RL_ENODEV, "no HIP device");
    std::vector<int> devs((size_t)n_dev);
    for (int d = 0; d < n_dev; ++d) {
        devs[d] = devices ? devices[d] : d;
        if (devs[d] < 0 || devs[d] >= ndev) return fail(RL_ENODEV, "device index out of range");
    }
    int cur = 0;
    const bool restore = hipGetDevice(&cur) == hipSuccess;
    const int nb = std::min(n_dev, B);             // no empty blocks
    const size_t mo = (size_t)cfg[0].max_outer_iters;
    const size_t N = (size_t)std::max(prob->N, 0);
    std::vector<rl_plan*> plans((size_t)nb, nullptr);
    auto release = [&](int code) {
        std::string e = g_err;
        for (rl_plan* q : plans) rl_plan_destroy(q);
        if (restore) hipSetDevice(cur);
        g_err = e;
        return code;
    };
    auto block = [&](int d, int& b0, int& b1) {
        b0 = (int)((int64_t)B * d / nb);
        b1 = (int)((int64_t)B * (d + 1) / nb);
    };
    int rc;
    for (int d = 0; d < nb; ++d) {
        int b0, b1;
        block(d, b0, b1);
        // every block takes the kernel shape rl_optimize would take for the whole batch, so
        // the results equal rl_optimize's bit for bit (the shapes' J / lap sum orders differ)
        if ((rc = rl_plan_create(&plans[d], devs[d], prob, n_cfg == 1 ? cfg : cfg + b0, n_cfg == 1 ? 1 : b1 - b0,
                                 seeds ? seeds + b0 : nullptr, b1 - b0, modes)) ||
            (rc = rl_plan_set_shape_batch(plans[d], B)) || (rc = rl_plan_run(plans[d], nullptr)))
            return release(rc);
    }
    // the caller's arrays from instance b0 on: every array moves by the bytes of b0 rows
    auto shifted = [&](const rl_out* o, int b0, rl_out& s) -> rl_out* {
        if (!o) return nullptr;
        s = *o;
        for (const OutField& f : kOutFields)
            if (f.out(s)) f.set_out(s, (char*)f.out(s) + f.bytes({(size_t)b0, N, mo, mo + 1}));
        return &s;
    };
    for (int d = 0; d < nb; ++d) {
        int b0, b1;
        block(d, b0, b1);
        rl_out smc, smt;
        if ((rc = rl_plan_fetch(plans[d], shifted(out_mincurv, b0, smc), shifted(out_mintime, b0, smt))))
            return release(rc);
    }
    return release(RL_OK);
}

}  // extern "C"
