// rl_host.h — what the host translation units of the C-ABI share (rl_abi.cpp, rl_plan.cpp,
// rl_stages.cpp, rl_cache.cpp): the error string, device selection, the ring image and its
// device copy, device-memory arenas, the result-field table, struct rl_plan and download
// jobs.  Host only: no kernel file includes it.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "rl_abi.h"
#include "rl_device.h"
#include "rl_kernels.h"
#include "rl_select.h"
#include "rl_lap_stage.h"
#include "rl_trajectory.h"
#include "rl_horizon.h"
#include "rl_rejoin.h"
#include "rl_query.h"
#include "rl_bounds.h"
#include "rl_rollout.h"

namespace rl {

// ------------------------------------------------------------------ errors, device
inline thread_local std::string g_err;          // rl_last_error

inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIPCHK(expr)                                                                  \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) return rl::fail(RL_EHIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
    } while (0)

// make `device` the calling thread's current device
inline int select_device(int32_t device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RL_ENODEV, "no HIP device");
    if (device < 0 || device >= ndev) return fail(RL_ENODEV, "device index out of range");
    HIPCHK(hipSetDevice(device));
    return RL_OK;
}

// variant: register-resident (N <= 4096) unless N is larger or RL_FORCE_STREAM=1 (testing)
inline bool use_stream(int N) {
    if (N > RL_REG_MAX_N) return true;
    const char* f = std::getenv("RL_FORCE_STREAM");
    return f && f[0] == '1';
}

inline int device_cus(int dev) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
    return n;
}

// ------------------------------------------------------------------ device memory
// The allocations of one owner and their total.  After a failed get() every later get()
// returns nullptr (err keeps the first failure) until release().  Nothing is smaller than
// 8 bytes, so a zero-length array still has an address of its own.
struct DevArena {
    std::vector<void*> ptrs;
    size_t bytes = 0;
    hipError_t err = hipSuccess;

    DevArena() = default;
    DevArena(const DevArena&) = delete;
    DevArena& operator=(const DevArena&) = delete;
    ~DevArena() { release(); }

    template <class T>
    T* get(size_t n) {
        if (err != hipSuccess) return nullptr;
        const size_t b = std::max<size_t>(n * sizeof(T), 8);
        void* q = nullptr;
        if ((err = hipMalloc(&q, b)) != hipSuccess) return nullptr;
        ptrs.push_back(q);
        bytes += b;
        return (T*)q;
    }
    bool ok() const { return err == hipSuccess; }
    void release() {
        for (void* q : ptrs) hipFree(q);
        ptrs.clear();
        bytes = 0;
        err = hipSuccess;
    }
};

// ------------------------------------------------------------------ rings
// std::max (ref:506 uses std::max(1e-30, ...))
inline double smax_h(double a, double b) { return (a < b) ? b : a; }

// Segment record from (x0,y0,x1,y1); vx,vy,denom exactly as the reference computes
// them (ref:482, 505-506).  mx,my,hr for conservative culling.
inline SegRec make_segrec(const double* q) {
    SegRec r;
    r.x0 = q[0];
    r.y0 = q[1];
    r.vx = q[2] - q[0];
    r.vy = q[3] - q[1];
    r.denom = smax_h(1e-30, r.vx * r.vx + r.vy * r.vy);
    r.mx = 0.5 * (q[0] + q[2]);
    r.my = 0.5 * (q[1] + q[3]);
    r.hr = 0.5 * std::sqrt(r.vx * r.vx + r.vy * r.vy) * (1.0 + 1e-9) + 1e-12;
    return r;
}

// Host image of one ring in the entry-stream form of rl_corridor.h: the vertices of
// each chain of consecutive segments (a segment starts a new chain unless its start
// equals the previous segment's end bit for bit), entry v holding the record of the
// segment that ends at v; padded to blocks of 32 with NaN entries.
struct RingHost {
    std::vector<double> vtx;        // [M][2]
    std::vector<SegRec> rec;        // [M]
    std::vector<uint32_t> flag;     // [M/32]
    std::vector<double> blk;        // [M/B][4] block circles (rl_corridor.h block culling)
    int M = 0, E = 0;
    double dl0 = 0, dl32 = 0;
};

inline RingHost make_ring(const double* s, int E) {
    RingHost R;
    R.E = E;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    SegRec dummy;
    dummy.x0 = dummy.y0 = dummy.vx = dummy.vy = dummy.mx = dummy.my = dummy.hr = nan;
    dummy.denom = 1.0;
    std::vector<char> ends;
    auto push = [&](double x, double y, const SegRec& r, bool end) {
        R.vtx.push_back(x);
        R.vtx.push_back(y);
        R.rec.push_back(r);
        ends.push_back(end);
    };
    double vmax = 0, rv = 0;
    bool nonfinite = false;        // std::max below drops a NaN second argument: tracked here
    for (int e = 0; e < E; ++e) {
        const double* q = s + 4 * e;
        for (int j = 0; j < 4; ++j) nonfinite |= !std::isfinite(q[j]);
        if (e == 0 || !(q[0] == s[4 * e - 2] && q[1] == s[4 * e - 1])) push(q[0], q[1], dummy, false);
        const SegRec r = make_segrec(q);
        push(q[2], q[3], r, true);
        vmax = std::max(vmax, std::fabs(r.vx) + std::fabs(r.vy));
        rv = std::max(rv, std::max(std::fabs(q[0]) + std::fabs(q[1]), std::fabs(q[2]) + std::fabs(q[3])));
    }
    while (ends.size() % 32) push(nan, nan, dummy, false);
    R.M = (int)ends.size();
    R.flag.assign(R.M / 32, 0u);
    for (int v = 0; v < R.M; ++v)
        if (ends[v]) R.flag[v / 32] |= 0x80000000u >> (v % 32);
    // A NaN/inf coordinate anywhere makes dl0/dl32 NaN: every pair of the ring is then a
    // candidate (rl_corridor.h `bad`) and the exact expressions propagate the values like
    // the reference
    R.dl0 = 4e-12 * (1.0 + vmax) + 4e-15 * rv;
    R.dl32 = 1e-6 * rv;
    if (nonfinite || !(vmax == vmax) || !(rv == rv)) R.dl0 = R.dl32 = nan;
    if (!(rv <= 1e30)) R.dl32 = INFINITY;          // beyond fp32 range: the fp32 filter keeps every pair
    // Per block of RL_BLK entries: a circle holding both endpoints of every segment that
    // ends in the block (the start point of the segment ending at v is entry v-1's
    // vertex, bit for bit). R = -1: no segment ends there; R = +inf: a non-finite
    // coordinate, so the block is never skipped.
    const int nb = R.M / RL_BLK;
    R.blk.assign((size_t)4 * nb, 0.0);
    for (int b = 0; b < nb; ++b) {
        double px[2 * RL_BLK], py[2 * RL_BLK];
        int n = 0;
        for (int v = b * RL_BLK; v < (b + 1) * RL_BLK; ++v) {
            if (!ends[v]) continue;
            px[n] = R.rec[v].x0; py[n++] = R.rec[v].y0;
            px[n] = R.vtx[2 * v]; py[n++] = R.vtx[2 * v + 1];
        }
        double* o = &R.blk[(size_t)4 * b];
        if (n == 0) { o[2] = -1.0; continue; }
        bool finite = true;
        double x0 = px[0], x1 = px[0], y0 = py[0], y1 = py[0];
        for (int j = 0; j < n; ++j) {
            finite = finite && std::isfinite(px[j]) && std::isfinite(py[j]);
            x0 = std::min(x0, px[j]); x1 = std::max(x1, px[j]);
            y0 = std::min(y0, py[j]); y1 = std::max(y1, py[j]);
        }
        const double cx = 0.5 * (x0 + x1), cy = 0.5 * (y0 + y1);
        double rad = 0.0;
        for (int j = 0; j < n; ++j) rad = std::max(rad, std::hypot(px[j] - cx, py[j] - cy));
        o[0] = cx;
        o[1] = cy;
        o[2] = finite ? rad * (1.0 + 1e-9) + 1e-12 * (1.0 + std::fabs(cx) + std::fabs(cy)) : INFINITY;
    }
    // fp32 copies for the side filter (rl_corridor.h ring_rays): vertices, then block
    // circles with the radius rounded up; packed after the fp64 circles
    std::vector<float> f32((size_t)2 * R.M + (size_t)4 * nb + (size_t)4 * R.M, 0.0f);
    for (int v = 0; v < 2 * R.M; ++v) f32[v] = (float)R.vtx[v];
    for (int b = 0; b < nb; ++b) {
        float* o = &f32[(size_t)2 * R.M + (size_t)4 * b];
        o[0] = (float)R.blk[(size_t)4 * b];
        o[1] = (float)R.blk[(size_t)4 * b + 1];
        const double rb = R.blk[(size_t)4 * b + 2];
        float rf = (float)rb;
        if ((double)rf < rb) rf = std::nextafter(rf, INFINITY);
        o[2] = rf;
    }
    for (int v = 0; v < R.M; ++v) {     // segment midpoints and half lengths (rounded up)
        float* o = &f32[(size_t)2 * R.M + (size_t)4 * nb + (size_t)4 * v];
        o[0] = (float)R.rec[v].mx;
        o[1] = (float)R.rec[v].my;
        const double hr = R.rec[v].hr;
        float hf = (float)hr;
        if ((double)hf < hr) hf = std::nextafter(hf, INFINITY);
        o[2] = hf;
    }
    const size_t n64 = R.blk.size();
    R.blk.resize(ring_blk_doubles((size_t)R.M), 0.0);
    std::memcpy(&R.blk[n64], f32.data(), f32.size() * sizeof(float));
    return R;
}

// The device copy of an (inner, outer) ring pair: each array holds the inner ring, then the
// outer one.  Owns nothing: the arrays belong to the arena they were taken from.
struct DevRing {
    double* vtx = nullptr;
    SegRec* rec = nullptr;
    uint32_t* flag = nullptr;
    double* blk = nullptr;
    int M[2] = {0, 0};
    double dl0[2] = {0, 0}, dl32[2] = {0, 0};

    // arrays for rh from `a`; false: a.err
    bool alloc(DevArena& a, const RingHost (&rh)[2]) {
        for (int r = 0; r < 2; ++r) { M[r] = rh[r].M; dl0[r] = rh[r].dl0; dl32[r] = rh[r].dl32; }
        const size_t Mt = (size_t)M[0] + M[1];
        vtx = a.get<double>(2 * Mt);
        rec = a.get<SegRec>(Mt);
        flag = a.get<uint32_t>(Mt / 32);
        blk = a.get<double>(ring_blk_doubles(Mt));
        return a.ok();
    }
    // copy rh up on st and wait for the copies: they read rh's vectors
    bool upload(const RingHost (&rh)[2], hipStream_t st) const {
        bool ok = true;
        for (int r = 0, off = 0; r < 2; off += rh[r].M, ++r) {
            const RingHost& R = rh[r];
            if (R.M == 0) continue;
            ok = ok &&
                 hipMemcpyAsync(vtx + 2 * (size_t)off, R.vtx.data(), R.vtx.size() * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess &&
                 hipMemcpyAsync(rec + off, R.rec.data(), R.rec.size() * sizeof(SegRec), hipMemcpyHostToDevice, st) == hipSuccess &&
                 hipMemcpyAsync(flag + off / 32, R.flag.data(), R.flag.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess &&
                 hipMemcpyAsync(blk + ring_blk_doubles((size_t)off), R.blk.data(), R.blk.size() * sizeof(double),
                                hipMemcpyHostToDevice, st) == hipSuccess;
        }
        return (hipStreamSynchronize(st) == hipSuccess) && ok;
    }
    // the kernels' ring parameters (KParams::ring, CorrParams::ring, GeomParams::ring)
    void fill(RingDesc (&ring)[2], int Ei, int Eo) const {
        for (int r = 0, off = 0; r < 2; off += M[r], ++r) {
            ring[r].vtx = (const double2*)(vtx + 2 * (size_t)off);
            ring[r].rec = rec + off;
            ring[r].flag = flag + off / 32;
            ring[r].blk = blk + ring_blk_doubles((size_t)off);
            ring[r].M = M[r];
            ring[r].E = r == 0 ? Ei : Eo;
            ring[r].dl0 = dl0[r];
            ring[r].dl32 = dl32[r];
        }
    }
};

// ------------------------------------------------------------------ result fields
struct ModeBufs {
    double *x = nullptr, *y = nullptr, *heading = nullptr, *kappa = nullptr, *alpha_total = nullptr,
           *alpha_last = nullptr, *v = nullptr, *ax = nullptr, *lap = nullptr, *nx = nullptr, *ny = nullptr;
    int32_t *evals = nullptr, *accepts = nullptr, *sweeps = nullptr;
    StreamBufs sb{};          // large-N variant only
};

// the arrays of `mb` as a launch's result and scratch arrays (written out: KParams also takes
// nx / ny, which no caller sees)
inline void set_bufs(KParams& kp, const ModeBufs& mb) {
    kp.x = mb.x; kp.y = mb.y; kp.heading = mb.heading; kp.kappa = mb.kappa;
    kp.alpha_total = mb.alpha_total; kp.alpha_last = mb.alpha_last;
    kp.v = mb.v; kp.ax = mb.ax; kp.lap = mb.lap; kp.nx = mb.nx; kp.ny = mb.ny;
    kp.evals = mb.evals; kp.accepts = mb.accepts; kp.sweeps = mb.sweeps;
}

// Rows and columns of a set of result arrays.  The optimisers' own: {B, N, mo, mo + 1}; the
// lap stage evaluates at max_outer_iters = 0: {B, N, 0, 1}.
struct Dims {
    size_t rows, N, mo, sweeps;
};
enum FieldShape { F_ROW_N, F_ROW_MO, F_ROW, F_ROW_SWEEPS };   // f64 [rows][N], i32 [rows][mo], f64 [rows], i32 [rows][sweeps]

// One result array: its member of rl_out and of ModeBufs, its shape, whether only the
// min-time optimiser writes it, and whether rl_plan_fetch_lap downloads it.
struct OutField {
    double* rl_out::*o64;
    int32_t* rl_out::*o32;
    double* ModeBufs::*b64;
    int32_t* ModeBufs::*b32;
    FieldShape shape;
    bool mintime, lap;

    constexpr OutField(double* rl_out::*o, double* ModeBufs::*b, FieldShape s, bool mt, bool lp)
        : o64(o), o32(nullptr), b64(b), b32(nullptr), shape(s), mintime(mt), lap(lp) {}
    constexpr OutField(int32_t* rl_out::*o, int32_t* ModeBufs::*b, FieldShape s, bool mt, bool lp)
        : o64(nullptr), o32(o), b64(nullptr), b32(b), shape(s), mintime(mt), lap(lp) {}

    void* out(const rl_out& o) const { return o64 ? (void*)(o.*o64) : (void*)(o.*o32); }
    void* buf(const ModeBufs& b) const { return b64 ? (void*)(b.*b64) : (void*)(b.*b32); }
    void set_out(rl_out& o, void* p) const {
        if (o64) o.*o64 = (double*)p;
        else o.*o32 = (int32_t*)p;
    }
    void set_buf(ModeBufs& b, void* p) const {
        if (b64) b.*b64 = (double*)p;
        else b.*b32 = (int32_t*)p;
    }
    size_t bytes(const Dims& d) const {
        return shape == F_ROW_N ? d.rows * d.N * 8 : shape == F_ROW_MO ? d.rows * d.mo * 4 :
               shape == F_ROW ? d.rows * 8 : d.rows * d.sweeps * 4;
    }
};
// In download order: download_staged and download_overlapped index events and staging
// offsets by job position.
constexpr OutField kOutFields[] = {
    {&rl_out::x, &ModeBufs::x, F_ROW_N, false, false},
    {&rl_out::y, &ModeBufs::y, F_ROW_N, false, false},
    {&rl_out::heading, &ModeBufs::heading, F_ROW_N, false, true},
    {&rl_out::kappa, &ModeBufs::kappa, F_ROW_N, false, true},
    {&rl_out::alpha_total, &ModeBufs::alpha_total, F_ROW_N, false, false},
    {&rl_out::alpha_last, &ModeBufs::alpha_last, F_ROW_N, false, false},
    {&rl_out::evals, &ModeBufs::evals, F_ROW_MO, false, false},
    {&rl_out::accepts, &ModeBufs::accepts, F_ROW_MO, false, false},
    {&rl_out::v, &ModeBufs::v, F_ROW_N, true, true},
    {&rl_out::ax, &ModeBufs::ax, F_ROW_N, true, true},
    {&rl_out::lap, &ModeBufs::lap, F_ROW, true, true},
    {&rl_out::vpass_sweeps, &ModeBufs::sweeps, F_ROW_SWEEPS, true, true},
};

// the result arrays of `mb` from `a` (min-time's too if `mintime`), none for an empty shape;
// callers pass the column counts they need allocated, not the ones they download
inline void alloc_fields(DevArena& a, ModeBufs& mb, const Dims& d, bool mintime) {
    for (const OutField& f : kOutFields)
        if ((mintime || !f.mintime) && f.bytes(d)) f.set_buf(mb, a.get<char>(f.bytes(d)));
}

// ------------------------------------------------------------------ downloads
// (host destination, device source, bytes)
struct CopyJob {
    void* dst;
    const void* src;
    size_t bytes;
};
inline void add_job(std::vector<CopyJob>& jobs, void* dst, const void* src, size_t bytes) {
    if (dst && src && bytes) jobs.push_back({dst, src, bytes});
}
// the copies that fill `o` from the arrays of `mb` (kOutFields order); lap_only: the fields
// rl_plan_fetch_lap downloads
inline void field_jobs(const rl_out* o, const ModeBufs& mb, const Dims& d, bool mintime, bool lap_only,
                       std::vector<CopyJob>& jobs) {
    if (!o) return;
    for (const OutField& f : kOutFields)
        if ((mintime || !f.mintime) && (f.lap || !lap_only)) add_job(jobs, f.out(*o), f.buf(mb), f.bytes(d));
}
// queue the jobs on st as device-to-host copies (the caller synchronises)
inline int queue_downloads(const std::vector<CopyJob>& jobs, hipStream_t st) {
    for (const CopyJob& j : jobs) {
        hipError_t e = hipMemcpyAsync(j.dst, j.src, j.bytes, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return fail(RL_EHIP, std::string("download: ") + hipGetErrorString(e));
    }
    return RL_OK;
}

// ------------------------------------------------------------------ pose-query stages
// The plan's side of one pose-query stage; a plan has one per QueryKind (rl_query.h).  The queries
// go up and the results come down as one packed block each (in, out; rl_query.h has their layout),
// through one pinned host block (pin) of the larger capacity; all three grow with Q, M_cap and
// K_cap.  Q, M, K (0 for the horizon) and C (the candidates per query of a fan stage, 0 for every
// other) are the last stage's Q, M_cap, K_cap and n_cand: with the stage's kind they give its
// layout again.  The fan stage has a scratch block on the device as well, which never comes down.
// Whether the stage holds results, and its events, are the plan's (rl_plan::valid, rl_plan::rec).
struct QueryStage {
    char *in = nullptr, *out = nullptr, *pin = nullptr, *scratch = nullptr;
    size_t in_cap = 0, out_cap = 0, scratch_cap = 0;
    DevArena mem;                     // in, out: they count toward the plan's dev_bytes()
    DevArena scratch_mem;             // scratch: it counts as well
    int Q = 0, M = 0, K = 0, C = 0;
    double dt = 0;                    // that stage's tick step (the bounds stage's tick kernel reads it)

    void release_blocks() {
        mem.release();
        if (pin) hipHostFree(pin);
        in = out = pin = nullptr;
        in_cap = out_cap = 0;
    }
    void release() {
        release_blocks();
        scratch_mem.release();
        scratch = nullptr;
        scratch_cap = 0;
    }
    // blocks of at least in_bytes and out_bytes; they only grow.  last_stream: the plan's, which
    // may still use the old ones.  `what` names the stage in the message.
    int reserve(hipStream_t last_stream, size_t in_bytes, size_t out_bytes, const char* what) {
        if (in && in_bytes <= in_cap && out_bytes <= out_cap) return RL_OK;
        if (last_stream) HIPCHK(hipStreamSynchronize(last_stream));
        const size_t ic = std::max(in_bytes, in_cap), oc = std::max(out_bytes, out_cap);
        release_blocks();
        char* d_in = mem.get<char>(ic);
        char* d_out = mem.get<char>(oc);
        void* host = nullptr;
        if (!mem.ok() || hipHostMalloc(&host, std::max(ic, oc), hipHostMallocDefault) != hipSuccess) {
            mem.release();
            return fail(RL_ENOMEM, std::string("allocation of the ") + what + " buffers failed");
        }
        in = d_in;
        out = d_out;
        pin = (char*)host;
        in_cap = ic;
        out_cap = oc;
        return RL_OK;
    }
    // a scratch block of at least `bytes`; it only grows
    int reserve_scratch(hipStream_t last_stream, size_t bytes, const char* what) {
        if (scratch && bytes <= scratch_cap) return RL_OK;
        if (last_stream) HIPCHK(hipStreamSynchronize(last_stream));
        scratch_mem.release();
        scratch_cap = 0;
        scratch = scratch_mem.get<char>(bytes);
        if (!scratch_mem.ok()) {
            scratch_mem.release();
            scratch = nullptr;
            return fail(RL_ENOMEM, std::string("allocation of the ") + what + " scratch block failed");
        }
        scratch_cap = bytes;
        return RL_OK;
    }
    size_t dev_bytes() const { return mem.bytes + scratch_mem.bytes; }
};

}  // namespace rl

// ------------------------------------------------------------------ the plan
// What the plan keeps per rl::Stage (rl_stage_graph.h): the events around its last enqueue and the
// stream it went to; created at the stage's first enqueue (stage_begin).  The run's events are
// rl_plan::ev, so its record holds a stream only.
struct StageRec {
    hipEvent_t ev[2] = {nullptr, nullptr};   // start (of an uploading stage: after the upload, which reads pin), end
    hipStream_t stream = nullptr;
};

struct rl_plan {
    int device = 0;
    int N = 0, B = 0, modes = 0, ncfg = 0, max_outer = 0, closed = 1, Ei = 0, Eo = 0;
    // batch size the kernel shape is chosen for (rl_plan_set_shape_batch; 0 = B): the
    // shapes sum J and the lap in different orders, so plans whose results must equal
    // each other's bit for bit use the same one (rl_optimize_multi: the whole call's B)
    int shape_B = 0;
    bool stream = false;              // streaming kernel (use_stream at creation)
    double L = 0, veh_width = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t last_stream = nullptr;
    // both modes in one run: the min-time kernel runs on aux_stream, concurrently with the
    // min-curvature kernel (the optimisers are independent); the run stream waits for it
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // run start, mode starts, run end
    hipEvent_t ev_end[2] = {nullptr, nullptr};                 // mode ends
    // The run and the twelve stages after it, by rl::Stage: which hold results (a stage's counts
    // below, traj_R, bnd_R, hb_Q, qs[k].Q and the like, are sizes and say nothing about that), and
    // each one's events and stream.  run_done, stage_begin and stage_end below keep them.
    rl::StageSet valid;
    StageRec rec[rl::N_STAGES];
    hipEvent_t ev_lap_mid = nullptr;                           // between the lap stage's two kernels (kernel_ms 5, 6)
    double* d_center = nullptr;
    double* d_Ls = nullptr;           // per-instance L (lap evaluation) or nullptr
    int64_t center_stride = 0;        // doubles between instances' centres (0: shared)
    rl::DevRing ring;
    rl_cfg* d_cfg = nullptr;
    uint64_t* d_seeds = nullptr;
    rl::ModeBufs mb[2];
    // per-mode instance completion flags of the next run (run_cached's overlapped
    // download; nullptr: none) and the value the kernel stores into them
    uint32_t* done[2] = {nullptr, nullptr};
    uint32_t epoch = 0;
    // outer iteration 0's corridor, cast once per run for the whole batch (KParams::lo0/hi0):
    // its bounds, the cfg margin all instances share (margin_uniform), and the event the
    // concurrent min-time stream waits for
    double *d_lo0 = nullptr, *d_hi0 = nullptr;
    double margin0 = 0;
    bool margin_uniform = false;
    hipEvent_t ev_c = nullptr;
    rl::DevArena mem;                 // everything above
    // selection stage (rl_plan_select): the scores of the last select, its winners and their
    // rows in compact buffers sized for sel_cap rows; allocated at the first select and again
    // when G*k outgrows sel_cap.
    double* d_score = nullptr;        // [B] min-curvature scores (min-time ranks mb[1].lap)
    int32_t* d_index = nullptr;       // [sel_cap]
    double* d_score_sel = nullptr;    // [sel_cap]
    rl::ModeBufs selb;                // compact rows (nx, ny, sb unused)
    rl::DevArena sel_mem;
    int sel_cap = 0, sel_mode = 0, sel_G = 0, sel_k = 0;
    const double* sel_scores = nullptr;   // the [B] scores the last select ranked
    bool sel_lap = false;             // the last select ranked the lap stage's lap (RL_SCORE_LAP)
    // lap stage (rl_plan_lap): the min-curvature rows packed as per-instance centres, their
    // own lengths, the plan's cfgs with max_outer_iters = 0, and the result and scratch arrays
    // of the min-time kernel that evaluates them; allocated at the first rl_plan_lap.
    double* d_lap_center = nullptr;   // [B][N][2]
    double* d_Lmc = nullptr;          // [B]
    rl_cfg* d_cfg_lap = nullptr;      // [ncfg]
    rl::ModeBufs lapb;                // sweeps [B][1]; evals / accepts unused
    rl::DevArena lap_mem;
    // trajectory stage (rl_plan_trajectory): the columns [traj_R][traj_M], the stamps
    // [traj_R][N + 1], T and count [traj_R] of the last stage, in buffers sized for traj_cap_R
    // rows of traj_cap_M ticks; allocated at the first stage and again when either grows.
    double* traj_col[rl::TRAJ_COLS] = {};
    double* traj_stamps = nullptr;
    double* traj_T = nullptr;
    int32_t* traj_count = nullptr;
    rl::DevArena traj_mem;
    int traj_cap_R = 0, traj_cap_M = 0, traj_R = 0, traj_M = 0;
    // pose-query stages (rl::QueryStage, one per rl::QueryKind): they read the last
    // trajectory stage through traj_q, that stage's launch parameters, which stay valid while
    // the stage is and the rows they point at are those the stamps were made from:
    // traj_sel_epoch / traj_lap_epoch are sel_epoch / lap_epoch (counted up by every selection /
    // lap stage) at that launch.  Each stage has blocks of its own, so the last horizon stage
    // stays fetchable after a rejoin, stop or retime stage and the other way round.
    rl::TrajParams traj_q{};
    int traj_mode = 0;
    uint32_t sel_epoch = 0, lap_epoch = 0, traj_sel_epoch = 0, traj_lap_epoch = 0;
    rl::QueryStage qs[rl::QUERY_KINDS];            // by kind
    rl::QueryStage& stage(rl::QueryKind k) { return qs[(int)k]; }
    // bounds stage (rl_plan_bounds, rl::BndParams): lo, hi, nx, ny [bnd_R][N] of the last
    // trajectory stage's rows, row for row, in buffers sized for bnd_cap_R rows.  Its tick kernel
    // (rl_plan_horizon_bounds) reads them and the last horizon stage's results: lo, hi
    // [hb_Q][hb_M] and lo0, hi0 [hb_Q] in buffers of hb_cap_QM and hb_cap_Q doubles.
    double* bnd[4] = {};              // lo, hi, nx, ny (rl_bnd's order)
    rl::DevArena bnd_mem;
    int bnd_cap_R = 0, bnd_R = 0;
    double* hb[4] = {};               // lo, hi, lo0, hi0 (rl_hzn_bnd's order)
    rl::DevArena hb_mem;
    size_t hb_cap_QM = 0, hb_cap_Q = 0;
    int hb_Q = 0, hb_M = 0;
    // rollout stage (rl_plan_rollouts, rl::RllParams): blocks and pinned staging of its own on the
    // pose-query stages' pattern (rl::RllLayout has their layout).  rll.M is the last stage's T,
    // rll_R its G*k.
    rl::QueryStage rll;
    int rll_R = 0;
    // the event that ends a stage's last enqueue (nullptr: never enqueued)
    hipEvent_t end_event(rl::Stage s) const { return s == rl::Stage::Run ? ev[3] : rec[(int)s].ev[1]; }

    template <class T>
    int alloc(T** p, size_t n) {
        *p = mem.get<T>(n);
        return *p ? RL_OK : nomem();
    }
    int nomem() const { return rl::fail(RL_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(mem.err)); }
    // device memory held (plan cache budget)
    size_t dev_bytes() const {
        size_t n = mem.bytes + sel_mem.bytes + lap_mem.bytes + traj_mem.bytes + bnd_mem.bytes + hb_mem.bytes;
        for (const auto& s : qs) n += s.dev_bytes();
        return n + rll.dev_bytes();
    }
    // the stream of the last run or stage
    hipStream_t run_stream() const { return last_stream ? last_stream : own_stream; }
    // the batch size the kernel shape is chosen for
    int shape_batch() const { return shape_B > 0 ? shape_B : B; }
};

namespace rl {

// ------------------------------------------------------------------ the plan's stages
// Make `st` wait for the last enqueue of stage `of`, unless that went to st itself, where stream
// order does the same; a stage never enqueued has nothing to wait for.
inline int stage_wait(rl_plan* p, Stage of, hipStream_t st) {
    const hipEvent_t e = p->end_event(of);
    if (e && p->rec[(int)of].stream != st) HIPCHK(hipStreamWaitEvent(st, e, 0));
    return RL_OK;
}
// Every stage's enqueue begins here, after its invalidate() and its allocations: the stage's events,
// st behind every stage it reads (kStages) and every stage of the mask `also`, the plan's last
// stream, and with `mark` the start event.  An uploading stage passes mark = false and records
// rec.ev[0] itself, behind its upload.
inline int stage_begin(rl_plan* p, Stage s, hipStream_t st, unsigned also = 0, bool mark = true) {
    StageRec& r = p->rec[(int)s];
    for (auto& e : r.ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    const unsigned from = stage_info(s).reads | also;
    for (int o = 0; o < N_STAGES; ++o)
        if (from >> o & 1u)
            if (int rc = stage_wait(p, (Stage)o, st)) return rc;
    p->last_stream = st;
    if (mark) HIPCHK(hipEventRecord(r.ev[0], st));
    return RL_OK;
}
// and ends here, behind its last launch
inline int stage_end(rl_plan* p, Stage s, hipStream_t st) {
    HIPCHK(hipEventRecord(p->rec[(int)s].ev[1], st));
    p->rec[(int)s].stream = st;
    p->valid.set(s);
    return RL_OK;
}
// the closing bookkeeping of a run on st, behind its end event: every stage is of an earlier run
inline void run_done(rl_plan* p, hipStream_t st) {
    p->valid.invalidate(Stage::Run);
    p->valid.set(Stage::Run);
    p->rec[(int)Stage::Run].stream = st;
}

// rl_plan.cpp
// argument checks shared by every entry point that builds or reuses a plan (no device call)
int check_inputs(const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg, int32_t B, int32_t modes,
                 const double* centers);
// rl_plan_create with optional per-instance centres [B][N][2] and lengths [B]
// (centers/Ls non-NULL: prob->center_xy and prob->L are ignored)
int plan_create_ex(rl_plan** out, int32_t device, const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg,
                   const uint64_t* seeds, int32_t B, int32_t modes, const double* centers, const double* Ls);
// result and scratch buffers of mode m (0: min-curv, 1: min-time); a no-op if present
int alloc_mode(rl_plan* p, int m);
// the cfg margin of outer iteration 0's guard, if every instance has the same one (bitwise)
void set_margin(rl_plan* p, const rl_cfg* cfg, int n_cfg);
// the copies that fill `o` from mode m's results
void out_jobs(const rl_plan* p, int m, const rl_out* o, std::vector<CopyJob>& jobs);

// rl_stages.cpp
// group checks shared by every selection entry point (no device call); *gs = the group size
int check_groups(int32_t B, int32_t group_size, int32_t k, int* gs);
int check_select(const rl_select* sel, int32_t B, int32_t N, int32_t modes, int* gs);
// the copies that download the last selection of p (out_jobs' order for the rows)
void sel_jobs(const rl_plan* p, int32_t* index, double* score, double* all_scores, const rl_out* o,
              std::vector<CopyJob>& jobs);
// argument checks shared by every trajectory entry point (no device call)
int check_traj(double dt, int32_t M_cap);
// the copies that download the last trajectory stage of p into the non-NULL fields of t
void traj_jobs(const rl_plan* p, const rl_traj* t, std::vector<CopyJob>& jobs);
// argument checks of the pose-query entry points (no device call): the kind's query, NULL-checked
// by the caller, against a trajectory stage of R rows of N samples
int check_query(QueryKind kind, const QueryView& q, int32_t R, int32_t N, int32_t closed);
// the kind's kernel on q, the blocks `in` and `out` (device) laid out as L, reading the trajectory
// stage src: rl_query.h's pointers, and for every kind but the horizon ax_max_at's constants.  bnd:
// the bounds rows lo, hi, nx, ny (device) of a kind that reads them; scratch: the fan stage's block
hipError_t query_launch(const QueryLayout& L, const QueryView& q, const TrajParams& src, char* in, char* out,
                        const double* const (&bnd)[4], char* scratch, hipStream_t st);
// The rollout stage's packed blocks.  in: xy [Q][T][2], v [Q][T] (if given), row, seg_hint [Q] (if
// given).  out: the head (progress, e_max, margin_min, cost [Q] f64; count, valid, first_out [Q]
// i32; order [R] i32, R = G*k), then the per-pose arrays (u, e, dist2, s, margin, vref [Q][T] f64;
// seg [Q][T] i32).  Every f64 array starts on a multiple of 8 bytes.
struct RllLayout {
    size_t Q, T, R;
    bool has_v, has_row, has_hint;
    size_t in_bytes, head_bytes, out_bytes;
};
RllLayout rll_layout(size_t Q, size_t T, size_t R, bool has_v, bool has_row, bool has_hint);
// argument checks of the rollout entry points (no device call): the query, NULL-checked by the
// caller, against a trajectory stage of R rows; *gs = the group size
int check_rollouts(const rl_rll_query& q, int32_t R, int* gs);
void rll_pack(const rl_rll_query& q, const RllLayout& L, char* block);
// the fields of o from the results' block; poses: the block holds the per-pose arrays as well
void rll_unpack(const char* block, const RllLayout& L, const rl_rll* o, bool poses);
bool rll_wants_poses(const rl_rll* o);
// the rollout kernel on q, then the rank kernel on its costs: the blocks `in` and `out` (device)
// laid out as L, reading the trajectory stage src and the bounds rows lo, hi (device)
hipError_t rll_launch(const RllLayout& L, const rl_rll_query& q, int gs, const TrajParams& src, const double* lo,
                      const double* hi, char* in, char* out, hipStream_t st);

}  // namespace rl
