// rl_plan.cpp — C-ABI implementation, part 2: plans.  Creation (device buffers, one HIP
// stream per plan, HIP events), the run and the group run, fetch, bound device outputs,
// HIP-event timing and the shape queries.
#include <array>

#include "rl_host.h"

using namespace rl;

namespace {

// waves of one instance in the kernel launch_optimize / launch_stream picks for (N, B, mode)
int waves_per_instance(int N, int B, bool mintime, bool stream, int cus) {
    if (stream) return (rl::stream_threads() + 63) / 64;      // rl_stream.hip
    const rl::Shape s = rl::pick_shape(N, B, mintime, cus);
    if (s.K <= 0) return 16;
    return (s.T + 63) / 64;
}

// the launch parameters of mode m (0: min-curv, 1: min-time) of plan p
void fill_kparams(const rl_plan* p, int m, int sB, bool pre0, rl::KParams& kp) {
    kp = rl::KParams{};
    kp.center = p->d_center;
    kp.center_stride = p->center_stride;
    kp.Ls = p->d_Ls;
    p->ring.fill(kp.ring, p->Ei, p->Eo);
    kp.cfg = p->d_cfg;
    kp.seeds = p->d_seeds;
    set_bufs(kp, p->mb[m]);
    kp.N = p->N; kp.Ei = p->Ei; kp.Eo = p->Eo; kp.ncfg = p->ncfg; kp.B = p->B; kp.closed = p->closed;
    kp.shape_B = sB;
    kp.L = p->L; kp.veh_width = p->veh_width;
    kp.done = p->done[m];
    kp.epoch = p->epoch;
    kp.lo0 = pre0 ? p->d_lo0 : nullptr;
    kp.hi0 = pre0 ? p->d_hi0 : nullptr;
}

// mode index of `which` if it is one mode of the plan, else -1
int mode_of(const rl_plan* p, int32_t which) {
    const int m = (which == RL_MODE_MINCURV) ? 0 : (which == RL_MODE_MINTIME ? 1 : -1);
    return (m < 0 || !(p->modes & which)) ? -1 : m;
}

}  // namespace

void rl::set_margin(rl_plan* p, const rl_cfg* cfg, int n_cfg) {
    p->margin0 = cfg[0].safety_margin_m;
    p->margin_uniform = true;
    for (int c = 1; c < n_cfg; ++c)
        if (std::memcmp(&cfg[c].safety_margin_m, &p->margin0, sizeof(double)) != 0) p->margin_uniform = false;
}

int rl::check_inputs(const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg, int32_t B, int32_t modes,
                     const double* centers) {
    if (!prob || !cfg) return fail(RL_EINVAL, "problem/cfg is NULL");
    if (B < 1) return fail(RL_EINVAL, "B must be >= 1");
    if (n_cfg != 1 && n_cfg != B) return fail(RL_EINVAL, "n_cfg must be 1 or B");
    if (prob->N < 0) return fail(RL_EINVAL, "N < 0");
    if ((modes & (RL_MODE_MINCURV | RL_MODE_MINTIME)) == 0 || (modes & ~3)) return fail(RL_EINVAL, "bad modes");
    // any L is accepted like the reference (h = L/N, ref:690); only the pointer is checked
    if (prob->N > 0 && !prob->center_xy && !centers) return fail(RL_EINVAL, "center_xy is NULL");
    if (prob->Ei < 0 || prob->Eo < 0 || (prob->Ei > 0 && !prob->inner_seg) || (prob->Eo > 0 && !prob->outer_seg))
        return fail(RL_EINVAL, "bad segments");
    const int mo = cfg[0].max_outer_iters;
    for (int c = 0; c < n_cfg; ++c) {
        if (cfg[c].max_outer_iters != mo) return fail(RL_EINVAL, "max_outer_iters must be equal across cfgs");
        if (cfg[c].max_outer_iters < 0 || cfg[c].max_inner_iters < 0 || cfg[c].max_vpass_iters < 0)
            return fail(RL_EINVAL, "negative iteration count");
    }
    if (prob->N > rl::RL_STREAM_MAX_N) return fail(RL_ETOOBIG, "N exceeds the streaming kernel (N <= 1048576)");
    return RL_OK;
}

int rl::plan_create_ex(rl_plan** out, int32_t device, const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg,
                       const uint64_t* seeds, int32_t B, int32_t modes, const double* centers, const double* Ls) {
    if (!out) return fail(RL_EINVAL, "plan out pointer is NULL");
    *out = nullptr;
    if (int rc0 = check_inputs(prob, cfg, n_cfg, B, modes, centers)) return rc0;
    const int mo = cfg[0].max_outer_iters;
    if (int rc0 = select_device(device)) return rc0;

    rl_plan* p = new rl_plan();
    p->device = device;
    p->N = prob->N;
    p->B = B;
    p->modes = modes;
    p->ncfg = n_cfg;
    p->max_outer = mo;
    p->closed = prob->closed ? 1 : 0;
    p->L = prob->L;
    p->veh_width = prob->veh_width;
    p->Ei = prob->Ei;
    p->Eo = prob->Eo;
    p->stream = use_stream(p->N);
    int rc = RL_OK;
    auto cleanup = [&](int code) {
        rl_plan_destroy(p);
        return code;
    };
    if (hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&p->aux_stream, hipStreamNonBlocking) != hipSuccess)
        return cleanup(fail(RL_EHIP, "hipStreamCreate failed"));
    for (auto& e : p->ev)
        if (hipEventCreate(&e) != hipSuccess) return cleanup(fail(RL_EHIP, "hipEventCreate failed"));
    for (auto& e : p->ev_end)
        if (hipEventCreate(&e) != hipSuccess) return cleanup(fail(RL_EHIP, "hipEventCreate failed"));
    if (hipEventCreateWithFlags(&p->ev_c, hipEventDisableTiming) != hipSuccess)
        return cleanup(fail(RL_EHIP, "hipEventCreate failed"));
    set_margin(p, cfg, n_cfg);

    const size_t N = (size_t)std::max(p->N, 1);
    const RingHost rh[2] = {make_ring(prob->inner_seg, prob->Ei), make_ring(prob->outer_seg, prob->Eo)};
    p->center_stride = centers ? (int64_t)2 * (int64_t)N : 0;
    if (Ls && (rc = p->alloc(&p->d_Ls, (size_t)B))) return cleanup(rc);
    if ((rc = p->alloc(&p->d_center, centers ? 2 * N * (size_t)B : 2 * N))) return cleanup(rc);
    if (!p->ring.alloc(p->mem, rh)) return cleanup(p->nomem());
    if ((rc = p->alloc(&p->d_cfg, (size_t)n_cfg)) || (rc = p->alloc(&p->d_seeds, (size_t)B)) ||
        (rc = p->alloc(&p->d_lo0, N)) || (rc = p->alloc(&p->d_hi0, N)))
        return cleanup(rc);
    hipStream_t st = p->own_stream;
    if (p->N > 0 && hipMemcpyAsync(p->d_center, centers ? centers : prob->center_xy,
                                   (centers ? (size_t)B : 1) * 2 * N * sizeof(double), hipMemcpyHostToDevice, st))
        return cleanup(fail(RL_EHIP, "upload center"));
    if (Ls && hipMemcpyAsync(p->d_Ls, Ls, (size_t)B * sizeof(double), hipMemcpyHostToDevice, st))
        return cleanup(fail(RL_EHIP, "upload L"));
    if (!p->ring.upload(rh, st)) return cleanup(fail(RL_EHIP, "upload rings"));
    if (hipMemcpyAsync(p->d_cfg, cfg, (size_t)n_cfg * sizeof(rl_cfg), hipMemcpyHostToDevice, st))
        return cleanup(fail(RL_EHIP, "upload cfg"));
    std::vector<uint64_t> sd((size_t)B, 0);
    if (seeds) std::memcpy(sd.data(), seeds, (size_t)B * sizeof(uint64_t));
    if (hipMemcpyAsync(p->d_seeds, sd.data(), (size_t)B * sizeof(uint64_t), hipMemcpyHostToDevice, st))
        return cleanup(fail(RL_EHIP, "upload seeds"));
    for (int m = 0; m < 2; ++m)
        if ((modes & (1 << m)) && (rc = alloc_mode(p, m))) return cleanup(rc);
    if (hipStreamSynchronize(st) != hipSuccess) return cleanup(fail(RL_EHIP, "upload sync"));
    *out = p;
    return RL_OK;
}

int rl::alloc_mode(rl_plan* p, int m) {
    ModeBufs& mb = p->mb[m];
    if (mb.nx) return RL_OK;
    const size_t B = (size_t)p->B, N = (size_t)std::max(p->N, 1), mo = (size_t)p->max_outer;
    // (rl_plan_run zeroes max(mo, 1) counters per instance when nothing iterates)
    alloc_fields(p->mem, mb, {B, N, std::max<size_t>(mo, 1), mo + 1}, m == 1);
    mb.nx = p->mem.get<double>(B * N);
    mb.ny = p->mem.get<double>(B * N);
    if (p->stream) mb.sb.base = p->mem.get<double>(B * N * rl::RL_STREAM_ARRAYS);   // [B][15][N]
    return p->mem.ok() ? RL_OK : p->nomem();
}

void rl::out_jobs(const rl_plan* p, int m, const rl_out* o, std::vector<CopyJob>& jobs) {
    const size_t mo = (size_t)p->max_outer;
    field_jobs(o, p->mb[m], {(size_t)p->B, (size_t)p->N, mo, mo + 1}, m == 1, false, jobs);
}

extern "C" {

int rl_plan_set_shape_batch(rl_plan* plan, int32_t shape_B) {
    if (!plan || shape_B < 0) return fail(RL_EINVAL, "rl_plan_set_shape_batch: bad argument");
    plan->shape_B = shape_B;
    return RL_OK;
}

int rl_plan_shape(rl_plan* plan, int32_t mode, int32_t* K, int32_t* T) {
    if (!plan || !K || !T || (mode != RL_MODE_MINCURV && mode != RL_MODE_MINTIME))
        return fail(RL_EINVAL, "rl_plan_shape: bad argument");
    if (plan->stream) { *K = 0; *T = rl::stream_threads(); return RL_OK; }
    const rl::Shape s = rl::pick_shape(std::max(plan->N, 1), plan->shape_batch(), mode == RL_MODE_MINTIME,
                                       device_cus(plan->device));
    *K = s.K;
    *T = s.T;
    return RL_OK;
}

int rl_plan_destroy(rl_plan* plan) {
    if (!plan) return RL_OK;
    hipSetDevice(plan->device);
    // every stream that may still run a kernel of this plan drains before its buffers go:
    // a run that failed after queueing the min-time kernel on aux_stream, but before the
    // run stream waited for it, leaves that kernel reading and writing them
    if (plan->last_stream) hipStreamSynchronize(plan->last_stream);
    if (plan->aux_stream) hipStreamSynchronize(plan->aux_stream);
    if (plan->own_stream) hipStreamSynchronize(plan->own_stream);
    plan->mem.release();
    plan->sel_mem.release();
    plan->lap_mem.release();
    plan->traj_mem.release();
    for (auto& s : plan->qs) s.release();
    plan->rll.release();
    plan->bnd_mem.release();
    plan->hb_mem.release();
    for (auto& r : plan->rec)
        for (auto& e : r.ev)
            if (e) hipEventDestroy(e);
    if (plan->ev_lap_mid) hipEventDestroy(plan->ev_lap_mid);
    for (auto& e : plan->ev)
        if (e) hipEventDestroy(e);
    for (auto& e : plan->ev_end)
        if (e) hipEventDestroy(e);
    if (plan->ev_c) hipEventDestroy(plan->ev_c);
    if (plan->own_stream) hipStreamDestroy(plan->own_stream);
    if (plan->aux_stream) hipStreamDestroy(plan->aux_stream);
    delete plan;
    return RL_OK;
}

int rl_plan_create(rl_plan** out, int32_t device, const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg,
                   const uint64_t* seeds, int32_t B, int32_t modes) {
    return plan_create_ex(out, device, prob, cfg, n_cfg, seeds, B, modes, nullptr, nullptr);
}

int rl_plan_run(rl_plan* p, void* hip_stream) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    HIPCHK(hipSetDevice(p->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->own_stream;
    p->last_stream = st;
    HIPCHK(hipEventRecord(p->ev[0], st));
    // Both modes: run the min-time kernel concurrently on the aux stream when one kernel
    // leaves the GPU partly idle (B x waves per instance below two waves per SIMD on every
    // CU: C4's 512 single-wave instances per track, the drop-in B=1).  Larger batches fill
    // the GPU with either kernel alone and run them one after the other (C3: concurrent
    // 74.2 ms vs 73.1 ms sequential).
    const int cus = device_cus(p->device);
    const int sB = p->shape_batch();
    const bool both = (p->modes & (RL_MODE_MINCURV | RL_MODE_MINTIME)) == (RL_MODE_MINCURV | RL_MODE_MINTIME) &&
                      (int64_t)p->B * std::max(waves_per_instance(p->N, sB, false, p->stream, cus),
                                               waves_per_instance(p->N, sB, true, p->stream, cus)) <=
                          (int64_t)8 * cus;
    // Outer iteration 0's corridor is the same for every instance (P = the shared centre, the
    // problem's veh_width, one cfg margin): cast it once here, rl_corridor_kernel, and let the
    // instances load it.  Only for batches that fill the GPU in a throughput shape (or the
    // streaming kernel): a latency-shape batch would wait for the extra launch longer than its
    // instances save (~1/14 of their corridor time).  RL_CORRIDOR0=0 turns it off (A/B, tests).
    const int first_m = (p->modes & RL_MODE_MINCURV) ? 0 : 1;
    bool pre0 = p->N > 0 && p->max_outer > 0 && p->center_stride == 0 && p->margin_uniform && p->B >= 2;
    if (pre0 && !p->stream) {
        pre0 = !(rl::pick_shape(p->N, sB, first_m == 1, cus) == rl::fit_shape(rl::LAT_SHAPES, p->N));
    }
    if (pre0) {
        const char* e = std::getenv("RL_CORRIDOR0");
        pre0 = !(e && e[0] == '0');
    }
    if (pre0) {
        HIPCHK(hipEventRecord(p->ev[1 + first_m], st));        // (inside the first mode's time)
        rl::CorrParams c{};
        c.center = p->d_center;
        c.N = p->N;
        c.closed = p->closed;
        p->ring.fill(c.ring, p->Ei, p->Eo);
        c.guard = p->veh_width * 0.5 + p->margin0;              // ref:706, as the kernels form it
        c.lo = p->d_lo0;
        c.hi = p->d_hi0;
        const hipError_t e = rl::launch_corridor(c, st);
        if (e != hipSuccess) return fail(RL_EHIP, std::string("corridor launch: ") + hipGetErrorString(e));
        HIPCHK(hipEventRecord(p->ev_c, st));
    }
    if (both) HIPCHK(hipStreamWaitEvent(p->aux_stream, pre0 ? p->ev_c : p->ev[0], 0));   // everything queued before
    for (int m = 0; m < 2; ++m) {
        if (!(p->modes & (1 << m))) continue;
        hipStream_t st_run = st;
        st = (both && m == 1) ? p->aux_stream : st_run;
        ModeBufs& mb = p->mb[m];
        if (p->N == 0 || p->max_outer == 0) {
            // ref:689 / 912 — N==0 returns an empty Result; zero the counters
            HIPCHK(hipMemsetAsync(mb.evals, 0, sizeof(int32_t) * p->B * std::max(p->max_outer, 1), st));
            HIPCHK(hipMemsetAsync(mb.accepts, 0, sizeof(int32_t) * p->B * std::max(p->max_outer, 1), st));
            if (m == 1) {
                HIPCHK(hipMemsetAsync(mb.lap, 0, sizeof(double) * p->B, st));
                HIPCHK(hipMemsetAsync(mb.sweeps, 0, sizeof(int32_t) * p->B * (p->max_outer + 1), st));
            }
            if (p->N == 0) {
                // no kernel: record the mode's events anyway, so rl_plan_kernel_ms(1 + m)
                // reports the (empty) interval instead of failing on an unrecorded event
                HIPCHK(hipEventRecord(p->ev[1 + m], st));
                HIPCHK(hipEventRecord(p->ev_end[m], st));
                st = st_run;
                continue;
            }
        }
        rl::KParams kp;
        fill_kparams(p, m, sB, pre0, kp);
        if (!(pre0 && m == first_m)) HIPCHK(hipEventRecord(p->ev[1 + m], st));
        hipError_t e = p->stream ? rl::launch_stream(kp, mb.sb, m == 1, st) : rl::launch_optimize(kp, m == 1, st);
        if (e != hipSuccess) return fail(RL_EHIP, std::string("kernel launch: ") + hipGetErrorString(e));
        HIPCHK(hipEventRecord(p->ev_end[m], st));
        st = st_run;
    }
    if (both) HIPCHK(hipStreamWaitEvent(st, p->ev_end[1], 0));
    HIPCHK(hipEventRecord(p->ev[3], st));
    run_done(p, st);
    return RL_OK;
}

// rl_plan_run of n plans (one device) as few launches as their shapes allow: every (plan,
// mode) whose kernel shape is a one-wave throughput shape (rl::group_shape) joins the group
// launch of its (mode, K, closed) class, up to RL_GROUP_MAX plans per launch; the
// other plans run as rl_plan_run on their own streams.  The launches run concurrently, each
// on a plan-owned stream after everything queued on `hip_stream`, which waits for all of
// them.  Results equal each plan's own rl_plan_run bit for bit (the same instance code, the
// plan's own shape); the batch-wide first corridor is left to the instances.  Every plan's
// rl_plan_kernel_ms(.., 0) is the whole group's run, its mode times its launch's.
int rl_plan_run_group(rl_plan* const* plans, int32_t n, void* hip_stream) {
    if (!plans || n < 1) return fail(RL_EINVAL, "rl_plan_run_group: no plans");
    for (int i = 0; i < n; ++i) {
        if (!plans[i]) return fail(RL_EINVAL, "rl_plan_run_group: a plan is NULL");
        if (plans[i]->device != plans[0]->device) return fail(RL_EINVAL, "rl_plan_run_group: plans on different devices");
        for (int j = 0; j < i; ++j)
            if (plans[j] == plans[i]) return fail(RL_EINVAL, "rl_plan_run_group: a plan is listed twice");
    }
    HIPCHK(hipSetDevice(plans[0]->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : plans[0]->own_stream;
    const int cus = device_cus(plans[0]->device);
    struct Item {
        rl_plan* p;
        int m;
    };
    // class key: mode, K, closed.  A launch whose plans include a ragged N (N % K != 0) runs
    // the ragged form for all of them (it covers every N, bit for bit): one launch per class
    // instead of two (C4: 4 launches, all concurrent at 4 HW queues; 13.25 against 13.52 ms
    // split by N % K, profiles/r06/c4_group.log)
    std::vector<std::pair<std::array<int, 3>, std::vector<Item>>> classes;
    std::vector<rl_plan*> solo;
    for (int i = 0; i < n; ++i) {
        rl_plan* p = plans[i];
        const int sB = p->shape_batch();
        bool ok = !p->stream && p->N > 0 && p->max_outer > 0 && (p->modes & 3);
        std::array<int, 3> key[2];
        for (int m = 0; m < 2 && ok; ++m) {
            if (!(p->modes & (1 << m))) continue;
            const rl::Shape s = rl::pick_shape(p->N, sB, m == 1, cus);
            ok = rl::group_shape(s);
            key[m] = {m, s.K, p->closed ? 1 : 0};
        }
        if (!ok) {
            solo.push_back(p);
            continue;
        }
        for (int m = 0; m < 2; ++m) {
            if (!(p->modes & (1 << m))) continue;
            auto it = std::find_if(classes.begin(), classes.end(), [&](const auto& c) { return c.first == key[m]; });
            if (it == classes.end()) {
                classes.push_back({key[m], {}});
                it = classes.end() - 1;
            }
            it->second.push_back({p, m});
        }
    }
    // the plans of a class longest first (by N): the grid dispatches its workgroups in order,
    // so its last ones are the shorter instances (C4 13.39 -> 13.14 ms, profiles/r06/c4_group.log)
    for (auto& c : classes)
        std::stable_sort(c.second.begin(), c.second.end(), [](const Item& x, const Item& y) { return x.p->N > y.p->N; });
    // the launches: class chunks of up to RL_GROUP_MAX plans, then the solo plans
    struct Launch {
        int cls;
        size_t i0;
        int cnt;
        hipStream_t ls;
    };
    std::vector<Launch> launches;
    std::vector<hipStream_t> pool;                   // grouped plans' own and aux streams
    for (auto& c : classes)
        for (const Item& it : c.second)
            for (hipStream_t x : {it.p->own_stream, it.p->aux_stream})
                if (std::find(pool.begin(), pool.end(), x) == pool.end()) pool.push_back(x);
    for (size_t ci = 0; ci < classes.size(); ++ci)
        for (size_t i0 = 0; i0 < classes[ci].second.size(); i0 += rl::RL_GROUP_MAX)
            launches.push_back({(int)ci, i0, (int)std::min<size_t>(rl::RL_GROUP_MAX, classes[ci].second.size() - i0),
                                pool[launches.size() % pool.size()]});
    // fork: every launch stream waits for what `hip_stream` has queued, before any launch
    // (a solo plan's rl_plan_run re-records its own events)
    hipEvent_t start = plans[0]->ev_c;               // (a disable-timing event of the group)
    HIPCHK(hipEventRecord(start, st));
    for (const Launch& L : launches) HIPCHK(hipStreamWaitEvent(L.ls, start, 0));
    for (rl_plan* p : solo) HIPCHK(hipStreamWaitEvent(p->own_stream, start, 0));
    for (int i = 0; i < n; ++i) {
        HIPCHK(hipEventRecord(plans[i]->ev[0], st));
        plans[i]->last_stream = st;
    }
    std::vector<hipEvent_t> ends;
    for (const Launch& L : launches) {
        const int m = classes[L.cls].first[0];
        const rl::Shape s{classes[L.cls].first[1], 64};
        const std::vector<Item>& items = classes[L.cls].second;
        rl::KGroup g{};
        g.n = L.cnt;
        int blocks = 0;
        bool ragged = false;
        for (int j = 0; j < L.cnt; ++j) {
            rl_plan* p = items[L.i0 + j].p;
            fill_kparams(p, m, p->shape_batch(), false, g.p[j]);
            g.start[j] = blocks;
            blocks += p->B;
            ragged |= p->N % s.K != 0;
        }
        for (int j = 0; j < L.cnt; ++j) HIPCHK(hipEventRecord(items[L.i0 + j].p->ev[1 + m], L.ls));
        const hipError_t e = rl::launch_optimize_group(g, s, classes[L.cls].first[2] != 0, ragged, m == 1, L.ls);
        if (e != hipSuccess) return fail(RL_EHIP, std::string("group launch: ") + hipGetErrorString(e));
        for (int j = 0; j < L.cnt; ++j) HIPCHK(hipEventRecord(items[L.i0 + j].p->ev_end[m], L.ls));
        ends.push_back(items[L.i0 + L.cnt - 1].p->ev_end[m]);
    }
    for (rl_plan* p : solo) {
        const int rc = rl_plan_run(p, p->own_stream);
        if (rc != RL_OK) return rc;
        ends.push_back(p->ev[3]);
        p->last_stream = st;
    }
    for (hipEvent_t e : ends) HIPCHK(hipStreamWaitEvent(st, e, 0));
    for (int i = 0; i < n; ++i) {
        HIPCHK(hipEventRecord(plans[i]->ev[3], st));
        run_done(plans[i], st);
    }
    return RL_OK;
}

// idx 0: the whole run; 1, 2: its kernels; from 3 on: the stage kStages gives the index to
// (include/rl_abi.h has the list), the lap stage with three of them
int rl_plan_kernel_ms(rl_plan* p, int32_t idx, float* ms) {
    if (!p || !ms || !p->valid.has(Stage::Run)) return fail(RL_EINVAL, "plan not run");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipEventSynchronize(p->ev[3]));
    hipEvent_t a, b;
    const int s = stage_of_ms(idx);
    if (idx == 0) { a = p->ev[0]; b = p->ev[3]; }
    else if (idx == 1 && (p->modes & RL_MODE_MINCURV)) { a = p->ev[1]; b = p->ev_end[0]; }
    else if (idx == 2 && (p->modes & RL_MODE_MINTIME)) { a = p->ev[2]; b = p->ev_end[1]; }
    else if (s > (int)Stage::Run && p->valid.has((Stage)s)) {
        const StageRec& r = p->rec[s];
        const int part = idx - kStages[s].ms_first;     // of the lap stage: 1 its preparation kernel, 2 its evaluation kernel
        a = part == 2 ? p->ev_lap_mid : r.ev[0];
        b = part == 1 ? p->ev_lap_mid : r.ev[1];
        HIPCHK(hipEventSynchronize(r.ev[1]));
    }
    else return fail(RL_EINVAL, "kernel index not in this plan");
    HIPCHK(hipEventElapsedTime(ms, a, b));
    return RL_OK;
}

int rl_plan_fetch(rl_plan* p, rl_out* out_mc, rl_out* out_mt) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if ((out_mc && !(p->modes & RL_MODE_MINCURV)) || (out_mt && !(p->modes & RL_MODE_MINTIME)))
        return fail(RL_EINVAL, "requested a mode the plan did not run");
    HIPCHK(hipSetDevice(p->device));
    hipStream_t st = p->run_stream();
    std::vector<CopyJob> jobs;
    out_jobs(p, 0, out_mc, jobs);
    out_jobs(p, 1, out_mt, jobs);
    if (int rc = queue_downloads(jobs, st)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    return RL_OK;
}

int rl_plan_bind_device_outputs(rl_plan* p, int32_t which, const rl_out* d) {
    if (!p || !d) return fail(RL_EINVAL, "NULL argument");
    const int m = mode_of(p, which);
    if (m < 0) return fail(RL_EINVAL, "mode not in plan");
    for (const OutField& f : kOutFields)
        if ((m == 1 || !f.mintime) && f.out(*d)) f.set_buf(p->mb[m], f.out(*d));
    return RL_OK;
}

int rl_plan_device_outputs(rl_plan* p, int32_t which, rl_out* d) {
    if (!p || !d) return fail(RL_EINVAL, "NULL argument");
    const int m = mode_of(p, which);
    if (m < 0) return fail(RL_EINVAL, "mode not in plan");
    std::memset(d, 0, sizeof(*d));
    for (const OutField& f : kOutFields) f.set_out(*d, f.buf(p->mb[m]));
    return RL_OK;
}

}  // extern "C"
