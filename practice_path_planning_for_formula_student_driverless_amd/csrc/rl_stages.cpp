// rl_stages.cpp — C-ABI implementation, part 3: the stages that follow a plan's run on the
// device.  Selection (rl_select.hip): score, rank and gather.  Lap stage (rl_lap_stage.hip,
// DESIGN §3i): the debug dump's "min-curv lap" for every instance of a plan.  Trajectory
// stage (rl_trajectory.hip): time stamps and the state at every control tick.
// Horizon stage (rl_horizon.hip): poses located on that stage's rows, and the next
// ticks from there.  Rejoin stage (rl_rejoin.hip): the same from the car's speed, along a
// reachable profile.  Stop stage (rl_stop.hip): the same under a brake envelope, up
// to a target sample.  Retime stage (rl_retime.hip): the reference's speed pass
// over the nodes ahead, under the car's cfg.  Recover stage (rl_recover.hip): a path
// from the car's offset back to the row inside the bounds stage's free width, and that speed pass
// on it.  Fan stage (rl_recover_fan.hip): the recover stage for C merge lengths per
// pose, and the best one served.  These six pose-query stages are the kinds of rl_query.h's table:
// they share one checked prologue, one enqueue (query_enqueue), one launch switch (query_launch) and
// one fetch (query_fetch), and their entry points are one-line forwards that name the kind.
// Bounds stage (rl_bounds.hip): the free track width about the trajectory stage's
// rows, and at the horizon stage's ticks.  Rollout stage (rl_rollout.hip): sampled
// trajectories located pose by pose on those rows, scored and ranked; a stage of its own beside the
// table, as the bounds stage is, because its arrays are [Q][T].
// Every stage is a rl::Stage of rl_stage_graph.h.  An enqueue is: the checks,
// plan->valid.invalidate(stage), which also clears every stage that reads this one, the allocation,
// stage_begin (events, the waits for the stages the table says it reads unless they ran on the same
// stream, the start event), the launches, stage_end (end event, stream, valid).  The uploading stages
// (the six kinds, the rollouts) share that as upload_launch; the fetches outside the query table
// share stage_fetch; traj_current refuses new readers of rows a later selection or lap stage replaced.
#include "rl_host.h"

using namespace rl;

int rl::check_groups(int32_t B, int32_t group_size, int32_t k, int* gs) {
    if (B < 1) return fail(RL_EINVAL, "select: B must be >= 1");
    if (group_size < 0) return fail(RL_EINVAL, "select: group_size < 0");
    const int g = group_size == 0 ? B : group_size;
    if (g > B || B % g != 0) return fail(RL_EINVAL, "select: B must be a multiple of group_size");
    if (k < 1) return fail(RL_EINVAL, "select: k must be >= 1");
    if (k > g) return fail(RL_EINVAL, "select: k exceeds group_size");
    if (k > RL_SELECT_MAX_K) return fail(RL_EINVAL, "select: k exceeds RL_SELECT_MAX_K (64)");
    *gs = g;
    return RL_OK;
}

int rl::check_select(const rl_select* sel, int32_t B, int32_t N, int32_t modes, int* gs) {
    if (!sel) return fail(RL_EINVAL, "select: sel is NULL");
    if (sel->mode != RL_MODE_MINCURV && sel->mode != RL_MODE_MINTIME)
        return fail(RL_EINVAL, "select: mode must be exactly one of RL_MODE_MINCURV, RL_MODE_MINTIME");
    if (!(modes & sel->mode)) return fail(RL_EINVAL, "select: mode is not among the plan's modes");
    if (int rc = check_groups(B, sel->group_size, sel->k, gs)) return rc;
    if (N == 0) return fail(RL_EINVAL, "select: N == 0 (nothing to rank)");
    return RL_OK;
}

// the copies of index / score / all_scores, then the winners' rows: the mode's own arrays,
// or (a min-curvature selection by lap) the lap stage's v, ax, lap and sweeps [R][1] as well
void rl::sel_jobs(const rl_plan* p, int32_t* index, double* score, double* all_scores, const rl_out* o,
                  std::vector<CopyJob>& jobs) {
    const size_t R = (size_t)p->sel_G * p->sel_k, mo = (size_t)p->max_outer;
    add_job(jobs, index, p->d_index, R * 4);
    add_job(jobs, score, p->d_score_sel, R * 8);
    add_job(jobs, all_scores, p->sel_scores, (size_t)p->B * 8);
    const bool mt = p->sel_mode == RL_MODE_MINTIME;
    field_jobs(o, p->selb, {R, (size_t)p->N, mo, mt ? mo + 1 : 1}, mt || p->sel_lap, false, jobs);
}

int rl::check_traj(double dt, int32_t M_cap) {
    if (!std::isfinite(dt) || !(dt > 0.0)) return fail(RL_EINVAL, "trajectory: dt must be finite and > 0");
    if (M_cap < 1 || M_cap > RL_TRAJ_MAX_TICKS) return fail(RL_EINVAL, "trajectory: M_cap must be 1..1048576");
    return RL_OK;
}

// the columns in rl_traj's order (TrajParams::out's), then stamps, T and count
void rl::traj_jobs(const rl_plan* p, const rl_traj* t, std::vector<CopyJob>& jobs) {
    if (!t) return;
    const size_t R = (size_t)p->traj_R, col = R * (size_t)p->traj_M * 8;
    double* const dst[TRAJ_COLS] = {t->s, t->x, t->y, t->heading, t->kappa, t->v, t->ax};
    for (int c = 0; c < TRAJ_COLS; ++c) add_job(jobs, dst[c], p->traj_col[c], col);
    add_job(jobs, t->stamps, p->traj_stamps, R * ((size_t)p->N + 1) * 8);
    add_job(jobs, t->T, p->traj_T, R * 8);
    add_job(jobs, t->count, p->traj_count, R * 4);
}

namespace {

// the horizon part of every kind's query: the sizes, and the rows and hints against a trajectory
// stage of R rows of N samples
int check_hzn(const rl_rjn_query& q, int32_t R, int32_t N, int32_t closed) {
    if (!q.pose_xy) return fail(RL_EINVAL, "horizon: the query or its pose_xy is NULL");
    if (q.Q < 1 || q.Q > RL_HZN_MAX_QUERIES) return fail(RL_EINVAL, "horizon: Q must be 1..65536");
    if (q.window < 0) return fail(RL_EINVAL, "horizon: window < 0");
    if (int rc = check_traj(q.dt, q.M_cap)) return rc;
    if (N < 1) return fail(RL_EINVAL, "horizon: N == 0 (no row)");
    const int32_t S = closed ? N : N - 1;
    for (int32_t k = 0; k < q.Q; ++k) {
        const int32_t r = q.row ? q.row[k] : 0, g = q.seg_hint ? q.seg_hint[k] : -1;
        if (r < 0 || r >= R) return fail(RL_EINVAL, "horizon: a row outside the trajectory stage's [0, R)");
        if (g < -1 || g >= S) return fail(RL_EINVAL, "horizon: a seg_hint outside [-1, S)");
    }
    return RL_OK;
}

// check_hzn's, then v0, cfg and K_cap
int check_rjn(const rl_rjn_query& q, int32_t R, int32_t N, int32_t closed) {
    if (int rc = check_hzn(q, R, N, closed)) return rc;
    if (!q.v0 || !q.cfg) return fail(RL_EINVAL, "rejoin: v0 or cfg is NULL");
    if (q.K_cap < 1 || q.K_cap > RL_RJN_MAX_NODES) return fail(RL_EINVAL, "rejoin: K_cap must be 1..1024");
    for (int32_t k = 0; k < q.Q; ++k)
        if (!std::isfinite(q.v0[k]) || q.v0[k] < 0.0) return fail(RL_EINVAL, "rejoin: a v0 that is not finite or is < 0");
    return RL_OK;
}

// check_rjn's, then stop_sample and v_target
int check_stp(const QueryView& q, int32_t R, int32_t N, int32_t closed) {
    if (int rc = check_rjn(q.rj, R, N, closed)) return rc;
    if (!q.stop_sample) return fail(RL_EINVAL, "stop: stop_sample is NULL");
    for (int32_t k = 0; k < q.rj.Q; ++k) {
        if (q.stop_sample[k] < 0 || q.stop_sample[k] >= N) return fail(RL_EINVAL, "stop: a stop_sample outside [0, N)");
        if (q.v_target && (!std::isfinite(q.v_target[k]) || q.v_target[k] < 0.0))
            return fail(RL_EINVAL, "stop: a v_target that is not finite or is < 0");
    }
    return RL_OK;
}

// check_rjn's with K_cap <= RL_RCV_MAX_NODES, then merge_len and dir_xy; with `fan` merge_len is
// [Q][n_cand], and n_cand and Q*n_cand are checked
int check_rcv(const QueryView& q, int32_t R, int32_t N, int32_t closed, bool fan) {
    const int32_t C = q.n_cand;
    if (int rc = check_rjn(q.rj, R, N, closed)) return rc;
    if (q.rj.K_cap > RL_RCV_MAX_NODES) return fail(RL_EINVAL, "recover: K_cap must be 1..512");
    if (!q.merge_len) return fail(RL_EINVAL, "recover: merge_len is NULL");
    if (fan && (C < 1 || C > RL_FAN_MAX_CAND)) return fail(RL_EINVAL, "recover fan: n_cand must be 1..16");
    if (fan && (int64_t)q.rj.Q * C > RL_HZN_MAX_QUERIES) return fail(RL_EINVAL, "recover fan: Q*n_cand must be <= 65536");
    const size_t per = fan ? (size_t)C : 1;
    for (int32_t k = 0; k < q.rj.Q; ++k) {
        for (size_t c = 0; c < per; ++c)
            if (!std::isfinite(q.merge_len[k * per + c]) || !(q.merge_len[k * per + c] > 0.0))
                return fail(RL_EINVAL, "recover: a merge_len that is not finite or is <= 0");
        if (q.dir_xy && (!std::isfinite(q.dir_xy[2 * (size_t)k]) || !std::isfinite(q.dir_xy[2 * (size_t)k + 1])))
            return fail(RL_EINVAL, "recover: a dir_xy that is not finite");
    }
    return RL_OK;
}

// query_pointers of q, reading the trajectory stage src, and for every kind but the horizon
// ax_max_at's constant prefixes, as the optimisers' VConst evaluates them
RjnParams query_params(const TrajParams& src, const rl_rjn_query& q, const QueryLayout& L, char* in, char* out) {
    RjnParams r = query_pointers(q, L, in, out);
    r.hz.src = src;
    if (!q.cfg) return r;                              // a horizon query
    const rl_cfg& C = *q.cfg;
    const double a_total = C.use_total_ge_lat ? smax_h(C.a_total_max, C.a_lat_max) : C.a_total_max;
    r.cfg.a_total2 = a_total * a_total;
    r.cfg.kFd = 0.5 * C.rho_air * C.Cd * C.A_front_m2;
    r.cfg.Fr = C.mass_kg * 9.81 * C.c_rr;
    r.cfg.mass = C.mass_kg; r.cfg.Pmax = C.P_max_W;
    r.cfg.acc_cap = C.a_long_acc_cap; r.cfg.brk_cap = C.a_long_brake_cap;
    return r;
}

}  // namespace

int rl::check_query(QueryKind kind, const QueryView& q, int32_t R, int32_t N, int32_t closed) {
    switch (kind) {
    case QueryKind::Horizon: return check_hzn(q.rj, R, N, closed);
    case QueryKind::Rejoin:
    case QueryKind::Retime: return check_rjn(q.rj, R, N, closed);
    case QueryKind::Stop: return check_stp(q, R, N, closed);
    case QueryKind::Recover: return check_rcv(q, R, N, closed, false);
    case QueryKind::Fan: return check_rcv(q, R, N, closed, true);
    }
    return fail(RL_EINVAL, "unknown pose-query stage");
}

hipError_t rl::query_launch(const QueryLayout& L, const QueryView& q, const TrajParams& src, char* in, char* out,
                            const double* const (&bnd)[4], char* scratch, hipStream_t st) {
    const RjnParams r = query_params(src, q.rj, L, in, out);
    switch (L.kind) {
    case QueryKind::Horizon: return rl::launch_horizon(r.hz, st);
    case QueryKind::Rejoin: return rl::launch_rejoin(r, st);
    case QueryKind::Stop: return rl::launch_stop(stop_pointers(r, L, in, out), st);
    case QueryKind::Retime: return rl::launch_retime(retime_pointers(r, *q.rj.cfg, L, out), st);
    case QueryKind::Recover:
    case QueryKind::Fan: {
        const RcvParams c = recover_pointers(retime_pointers(r, *q.rj.cfg, L, out), q.dir_xy != nullptr, L, in, out, bnd);
        return L.kind == QueryKind::Fan ? rl::launch_recover_fan(fan_pointers(c, *q.rj.cfg, L, out, scratch), st)
                                        : rl::launch_recover(c, st);
    }
    }
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------------ the rollout stage's blocks
namespace {

size_t up8(size_t n) { return (n + 7) & ~(size_t)7; }

// the arrays of the results' block laid out as L, from its base: f64 [Q] x4, i32 [Q] x3, order
// [R]; then f64 [Q][T] x6 and seg [Q][T]
struct RllOut {
    char *head[RLL_HEAD_F64], *ihead[RLL_HEAD_I32], *order, *pose[RLL_POSE_F64], *seg;
};
RllOut rll_out(const RllLayout& L, char* base) {
    RllOut o;
    char* c = base;
    for (auto& a : o.head) { a = c; c += L.Q * 8; }
    for (auto& a : o.ihead) { a = c; c += L.Q * 4; }
    o.order = c;
    c = base + L.head_bytes;
    for (auto& a : o.pose) { a = c; c += L.Q * L.T * 8; }
    o.seg = c;
    return o;
}

}  // namespace

RllLayout rl::rll_layout(size_t Q, size_t T, size_t R, bool has_v, bool has_row, bool has_hint) {
    RllLayout L{Q, T, R, has_v, has_row, has_hint, 0, 0, 0};
    L.in_bytes = up8(Q * T * 8 * (has_v ? 3 : 2) + Q * 4 * ((has_row ? 1 : 0) + (has_hint ? 1 : 0)));
    L.head_bytes = up8(Q * 8 * RLL_HEAD_F64 + Q * 4 * RLL_HEAD_I32 + R * 4);
    L.out_bytes = L.head_bytes + up8(Q * T * 8 * RLL_POSE_F64 + Q * T * 4);
    return L;
}

int rl::check_rollouts(const rl_rll_query& q, int32_t R, int* gs) {
    if (!q.xy) return fail(RL_EINVAL, "rollouts: the query or its xy is NULL");
    if (q.Q < 1 || q.Q > RL_RLL_MAX_ROLLOUTS) return fail(RL_EINVAL, "rollouts: Q must be 1..65536");
    if (q.T < 1 || q.T > RL_RLL_MAX_STEPS) return fail(RL_EINVAL, "rollouts: T must be 1..512");
    if ((int64_t)q.Q * q.T > RL_RLL_MAX_POSES) return fail(RL_EINVAL, "rollouts: Q*T must be <= 4194304");
    if (q.window0 < 0 || q.window < 0) return fail(RL_EINVAL, "rollouts: window0 or window < 0");
    for (double w : {q.w_e, q.w_out, q.w_v, q.w_prog})
        if (!std::isfinite(w) || w < 0.0) return fail(RL_EINVAL, "rollouts: a weight that is not finite or is < 0");
    const int g = q.group_size == 0 ? q.Q : q.group_size;
    if (g < 1 || g > q.Q || q.Q % g != 0) return fail(RL_EINVAL, "rollouts: Q must be a multiple of group_size");
    if (q.k < 1 || q.k > g || q.k > RL_SELECT_MAX_K) return fail(RL_EINVAL, "rollouts: k must be 1..min(group_size, 64)");
    for (int32_t k = 0; k < q.Q; ++k) {
        if (q.row && (q.row[k] < 0 || q.row[k] >= R)) return fail(RL_EINVAL, "rollouts: a row outside the trajectory stage's [0, R)");
        if (q.seg_hint && q.seg_hint[k] < -1) return fail(RL_EINVAL, "rollouts: a seg_hint < -1");
    }
    *gs = g;
    return RL_OK;
}

void rl::rll_pack(const rl_rll_query& q, const RllLayout& L, char* block) {
    const size_t QT = L.Q * L.T;
    char* c = block;
    std::memcpy(c, q.xy, QT * 16); c += QT * 16;
    if (L.has_v) { std::memcpy(c, q.v, QT * 8); c += QT * 8; }
    if (L.has_row) { std::memcpy(c, q.row, L.Q * 4); c += L.Q * 4; }
    if (L.has_hint) std::memcpy(c, q.seg_hint, L.Q * 4);
}

bool rl::rll_wants_poses(const rl_rll* o) {
    return o->seg || o->u || o->e || o->dist2 || o->s || o->margin || o->vref;
}

void rl::rll_unpack(const char* block, const RllLayout& L, const rl_rll* o, bool poses) {
    const RllOut b = rll_out(L, const_cast<char*>(block));
    auto take = [](void* dst, const char* src, size_t bytes) {
        if (dst && bytes) std::memcpy(dst, src, bytes);
    };
    double* const head[RLL_HEAD_F64] = {o->progress, o->e_max, o->margin_min, o->cost};
    int32_t* const ihead[RLL_HEAD_I32] = {o->count, o->valid, o->first_out};
    for (int c = 0; c < RLL_HEAD_F64; ++c) take(head[c], b.head[c], L.Q * 8);
    for (int c = 0; c < RLL_HEAD_I32; ++c) take(ihead[c], b.ihead[c], L.Q * 4);
    take(o->order, b.order, L.R * 4);
    if (!poses) return;
    double* const pose[RLL_POSE_F64] = {o->u, o->e, o->dist2, o->s, o->margin, o->vref};
    for (int c = 0; c < RLL_POSE_F64; ++c) take(pose[c], b.pose[c], L.Q * L.T * 8);
    take(o->seg, b.seg, L.Q * L.T * 4);
}

hipError_t rl::rll_launch(const RllLayout& L, const rl_rll_query& q, int gs, const TrajParams& src, const double* lo,
                          const double* hi, char* in, char* out, hipStream_t st) {
    const size_t QT = L.Q * L.T;
    const RllOut b = rll_out(L, out);
    RllParams p{};
    p.src = src;
    p.lo = lo; p.hi = hi;
    char* c = in;
    p.xy = (const double*)c; c += QT * 16;
    if (L.has_v) { p.v = (const double*)c; c += QT * 8; }
    if (L.has_row) { p.row = (const int32_t*)c; c += L.Q * 4; }
    if (L.has_hint) p.hint = (const int32_t*)c;
    p.seg = (int32_t*)b.seg;
    for (int a = 0; a < RLL_POSE_F64; ++a) p.pose[a] = (double*)b.pose[a];
    for (int a = 0; a < RLL_HEAD_F64; ++a) p.head[a] = (double*)b.head[a];
    for (int a = 0; a < RLL_HEAD_I32; ++a) p.ihead[a] = (int32_t*)b.ihead[a];
    p.w_e = q.w_e; p.w_out = q.w_out; p.w_v = q.w_v; p.w_prog = q.w_prog;
    p.Q = q.Q; p.T = q.T; p.window0 = q.window0; p.window = q.window; p.hard_bounds = q.hard_bounds ? 1 : 0;
    const hipError_t e = rl::launch_rollouts(p, st);
    if (e != hipSuccess) return e;
    return rl::launch_rank(p.head[3], q.Q, gs, q.k, (int32_t*)b.order, nullptr, st);   // cost, rl_rank_scores' order
}

namespace {

// plan-owned trajectory buffers for R rows of M ticks; they count toward dev_bytes()
int traj_alloc(rl_plan* p, int R, int M) {
    if (p->traj_stamps && R <= p->traj_cap_R && M <= p->traj_cap_M) return RL_OK;
    if (p->last_stream) HIPCHK(hipStreamSynchronize(p->last_stream));   // it may still write the old ones
    DevArena& a = p->traj_mem;
    a.release();
    R = std::max(R, p->traj_cap_R);
    M = std::max(M, p->traj_cap_M);
    p->traj_cap_R = p->traj_cap_M = 0;
    p->traj_stamps = nullptr;
    for (auto& c : p->traj_col) c = a.get<double>((size_t)R * (size_t)M);
    double* stamps = a.get<double>((size_t)R * ((size_t)p->N + 1));
    p->traj_T = a.get<double>((size_t)R);
    p->traj_count = a.get<int32_t>((size_t)R);
    if (!a.ok()) {
        a.release();
        return fail(RL_ENOMEM, "hipMalloc (trajectory buffers) failed");
    }
    p->traj_stamps = stamps;
    p->traj_cap_R = R;
    p->traj_cap_M = M;
    return RL_OK;
}

// plan-owned selection buffers for `rows` winners; they count toward dev_bytes()
int select_alloc(rl_plan* p, int rows) {
    if (p->d_index && rows <= p->sel_cap) return RL_OK;
    if (p->last_stream) HIPCHK(hipStreamSynchronize(p->last_stream));   // it may still read the old ones
    DevArena& a = p->sel_mem;
    a.release();
    p->sel_cap = 0;
    p->selb = ModeBufs{};
    const size_t R = (size_t)rows, mo = (size_t)p->max_outer;
    p->d_score = a.get<double>((size_t)p->B);
    p->d_index = a.get<int32_t>(R);
    p->d_score_sel = a.get<double>(R);
    alloc_fields(a, p->selb, {R, (size_t)std::max(p->N, 1), std::max<size_t>(mo, 1), mo + 1}, true);
    if (!a.ok()) return fail(RL_ENOMEM, "hipMalloc (selection buffers) failed");
    p->sel_cap = rows;
    return RL_OK;
}

// plan-owned lap-stage buffers; they count toward dev_bytes()
int lap_alloc(rl_plan* p) {
    if (p->d_lap_center) return RL_OK;
    DevArena& a = p->lap_mem;
    const size_t B = (size_t)p->B, N = (size_t)std::max(p->N, 1), BN = B * N;
    ModeBufs& s = p->lapb;
    double* center = a.get<double>(2 * BN);
    p->d_Lmc = a.get<double>(B);
    p->d_cfg_lap = a.get<rl_cfg>((size_t)p->ncfg);
    alloc_fields(a, s, {B, N, 0, 1}, true);            // no outer iteration: no evals / accepts
    s.nx = a.get<double>(BN);
    s.ny = a.get<double>(BN);
    if (p->stream) s.sb.base = a.get<double>(BN * rl::RL_STREAM_ARRAYS);
    if (!a.ok()) {
        a.release();
        p->lapb = ModeBufs{};
        p->d_Lmc = nullptr;
        p->d_cfg_lap = nullptr;
        return fail(RL_ENOMEM, "hipMalloc (lap-stage buffers) failed");
    }
    p->d_lap_center = center;
    return RL_OK;
}

// rl_plan_select / rl_plan_select_scored (arguments checked).  by_lap: rank the lap stage's
// lap instead of the min-curvature score, and gather its v, ax, lap and sweeps as well.
int select_impl(rl_plan* p, const rl_select* sel, int gs, bool by_lap, void* hip_stream) {
    HIPCHK(hipSetDevice(p->device));
    const int m = sel->mode == RL_MODE_MINTIME ? 1 : 0;
    const int k = sel->k, G = p->B / gs, rows = G * k;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->run_stream();
    p->valid.invalidate(Stage::Select);
    ++p->sel_epoch;                                    // d_index and the compact rows change
    if (int rc = select_alloc(p, rows)) return rc;
    if (int rc = stage_begin(p, Stage::Select, st, by_lap ? sbit(Stage::Lap) : 0)) return rc;
    const ModeBufs& mb = p->mb[m];
    hipError_t e = hipSuccess;
    const double* scores = by_lap ? p->lapb.lap : mb.lap;   // min-time: the lap the optimiser wrote
    if (m == 0 && !by_lap) {
        e = rl::launch_score(mb.kappa, p->N, p->B, p->L, p->d_Ls, p->d_score, st);
        if (e != hipSuccess) return fail(RL_EHIP, std::string("score launch: ") + hipGetErrorString(e));
        scores = p->d_score;
    }
    e = rl::launch_rank(scores, p->B, gs, k, p->d_index, p->d_score_sel, st);
    if (e != hipSuccess) return fail(RL_EHIP, std::string("rank launch: ") + hipGetErrorString(e));
    const ModeBufs& sb = p->selb;
    rl::GatherParams g{};
    int c = 0;                                         // the [B][N] arrays, in kOutFields order
    for (const OutField& f : kOutFields)
        if (f.shape == F_ROW_N) {
            g.src[c] = mb.*f.b64;
            g.dst[c++] = sb.*f.b64;
        }
    g.lap_src = mb.lap; g.lap_dst = sb.lap;
    g.evals_src = mb.evals; g.evals_dst = sb.evals;
    g.accepts_src = mb.accepts; g.accepts_dst = sb.accepts;
    g.sweeps_src = mb.sweeps; g.sweeps_dst = sb.sweeps;
    g.index = p->d_index;
    g.N = p->N; g.B = p->B; g.mo = p->max_outer; g.rows = rows;
    e = rl::launch_gather(g, st);
    if (e != hipSuccess) return fail(RL_EHIP, std::string("gather launch: ") + hipGetErrorString(e));
    if (by_lap) {
        // a second gather: the lap stage's v, ax, lap and sweeps [B][1] of the same winners
        const ModeBufs& lb = p->lapb;
        rl::GatherParams h{};
        h.src[6] = lb.v; h.dst[6] = sb.v;
        h.src[7] = lb.ax; h.dst[7] = sb.ax;
        h.lap_src = lb.lap; h.lap_dst = sb.lap;
        h.sweeps_src = lb.sweeps; h.sweeps_dst = sb.sweeps;
        h.index = p->d_index;
        h.N = p->N; h.B = p->B; h.mo = 0; h.rows = rows;
        e = rl::launch_gather(h, st);
        if (e != hipSuccess) return fail(RL_EHIP, std::string("gather launch: ") + hipGetErrorString(e));
    }
    p->sel_mode = sel->mode;
    p->sel_lap = by_lap;
    p->sel_G = G;
    p->sel_k = k;
    p->sel_scores = scores;
    return stage_end(p, Stage::Select, st);
}

// Whether the rows the last trajectory stage read are still the ones its stamps were made from; a
// later selection or lap stage leaves that stage and what was enqueued on it fetchable, and refuses
// new readers of the rows, here.  fn: the entry point that asks.
int traj_current(const rl_plan* p, const std::string& fn) {
    if (p->traj_q.index && p->traj_sel_epoch != p->sel_epoch)
        return fail(RL_EINVAL, fn + ": a selection has replaced the winners the trajectory stage read");
    if (p->traj_mode == RL_MODE_MINCURV && p->traj_lap_epoch != p->lap_epoch)
        return fail(RL_EINVAL, fn + ": a lap stage has rewritten the rows the trajectory stage read");
    return RL_OK;
}

// The enqueue of a stage whose queries go up in one block (the pose-query kinds, the rollouts): the
// blocks of s for a layout L, pack(pin), the upload, then launch(), on st; s's sizes are the
// caller's to set.  The start event is recorded behind the upload, which reads the pinned block.
template <class Layout, class Pack, class Launch>
int upload_launch(rl_plan* p, Stage stage, QueryStage& s, const Layout& L, size_t scratch_bytes, hipStream_t st, Pack pack,
                  Launch launch) {
    const char* name = stage_info(stage).name;
    StageRec& r = p->rec[(int)stage];
    // An earlier upload may still read the pinned block, also one whose stage a run, a
    // trajectory stage or a failed launch has invalidated since (an event that was never
    // recorded is complete).
    if (r.ev[0]) HIPCHK(hipEventSynchronize(r.ev[0]));
    p->valid.invalidate(stage);
    if (int rc = s.reserve(p->last_stream, L.in_bytes, L.out_bytes, name)) return rc;
    if (scratch_bytes)
        if (int rc = s.reserve_scratch(p->last_stream, scratch_bytes, name)) return rc;
    if (int rc = stage_begin(p, stage, st, 0, false)) return rc;
    pack(s.pin);
    HIPCHK(hipMemcpyAsync(s.in, s.pin, L.in_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(r.ev[0], st));
    const hipError_t e = launch();
    if (e != hipSuccess) return fail(RL_EHIP, std::string(name) + " launch: " + hipGetErrorString(e));
    return stage_end(p, stage, st);
}

// every pose-query stage's rl_plan_<name> (arguments checked; a kind that reads the bounds stage
// after a valid one): one launch of the kind's kernel on the last trajectory stage
int query_enqueue(rl_plan* p, QueryKind kind, const QueryView& q, void* hip_stream) {
    QueryStage& s = p->stage(kind);
    if (int rc = traj_current(p, std::string("rl_plan_") + kind_info(kind).name)) return rc;
    HIPCHK(hipSetDevice(p->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->run_stream();
    const QueryLayout L = query_layout_of(kind, q);
    const int rc = upload_launch(
        p, stage_of(kind), s, L, L.scratch_bytes, st, [&](char* pin) { query_pack(q, L, pin); },
        [&] { return query_launch(L, q, p->traj_q, s.in, s.out, {p->bnd[0], p->bnd[1], p->bnd[2], p->bnd[3]}, s.scratch, st); });
    if (rc) return rc;
    s.Q = q.rj.Q;
    s.M = q.rj.M_cap;
    s.K = q.rj.K_cap;
    s.C = q.n_cand;
    s.dt = q.rj.dt;
    return RL_OK;
}

// plan-owned bounds buffers for R rows; they count toward dev_bytes()
int bounds_alloc(rl_plan* p, int R) {
    if (p->bnd[0] && R <= p->bnd_cap_R) return RL_OK;
    if (p->last_stream) HIPCHK(hipStreamSynchronize(p->last_stream));   // it may still use the old ones
    DevArena& a = p->bnd_mem;
    a.release();
    p->bnd_cap_R = 0;
    for (auto& b : p->bnd) b = a.get<double>((size_t)R * (size_t)p->N);
    if (!a.ok()) {
        a.release();
        for (auto& b : p->bnd) b = nullptr;
        return fail(RL_ENOMEM, "hipMalloc (bounds buffers) failed");
    }
    p->bnd_cap_R = R;
    return RL_OK;
}

// plan-owned buffers of the bounds at Q queries' M ticks each; they count toward dev_bytes()
int horizon_bounds_alloc(rl_plan* p, size_t Q, size_t M) {
    if (p->hb[0] && Q * M <= p->hb_cap_QM && Q <= p->hb_cap_Q) return RL_OK;
    if (p->last_stream) HIPCHK(hipStreamSynchronize(p->last_stream));
    DevArena& a = p->hb_mem;
    a.release();
    const size_t QM = std::max(Q * M, p->hb_cap_QM), Qc = std::max(Q, p->hb_cap_Q);
    p->hb_cap_QM = p->hb_cap_Q = 0;
    for (int c = 0; c < 4; ++c) p->hb[c] = a.get<double>(c < 2 ? QM : Qc);
    if (!a.ok()) {
        a.release();
        for (auto& b : p->hb) b = nullptr;
        return fail(RL_ENOMEM, "hipMalloc (horizon bounds buffers) failed");
    }
    p->hb_cap_QM = QM;
    p->hb_cap_Q = Qc;
    return RL_OK;
}

// every pose-query stage's rl_plan_fetch_<name> (a valid stage of `kind`; o: the kind's results
// struct): the results' block comes down through the pinned block, without the node arrays if o
// asks for none
int query_fetch(rl_plan* p, QueryKind kind, const void* o) {
    QueryStage& s = p->stage(kind);
    HIPCHK(hipSetDevice(p->device));
    hipStream_t st = p->run_stream();
    if (int rc = stage_wait(p, stage_of(kind), st)) return rc;   // (a later stage may have moved to another stream)
    const QueryLayout L = query_layout_of(kind, (size_t)s.Q, (size_t)s.M, (size_t)s.K, (size_t)s.C);
    HIPCHK(hipMemcpyAsync(s.pin, s.out, query_wants_nodes(kind, o) ? L.out_bytes : L.head_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    query_unpack(s.pin, L, o);
    return RL_OK;
}

// the fetch of a stage outside the query table (a valid one): the jobs on the plan's stream, behind
// the stage's end, and the wait for them
int stage_fetch(rl_plan* p, Stage stage, const std::vector<CopyJob>& jobs) {
    HIPCHK(hipSetDevice(p->device));
    hipStream_t st = p->run_stream();
    if (int rc = stage_wait(p, stage, st)) return rc;   // (a later stage may have moved to another stream)
    if (int rc = queue_downloads(jobs, st)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    return RL_OK;
}

// the checked prologue of every rl_plan_<name>: blocks of the kind's own, so every other stage
// stays as it is; a kind that reads the bounds stage reads its rows where they lie
template <QueryKind kind, class Query>
int plan_stage(rl_plan* p, const Query* query, void* hip_stream) {
    const KindInfo& k = kind_info(kind);
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (!query) return fail(RL_EINVAL, k.null_query);
    const std::string fn = std::string("rl_plan_") + k.name;
    if (!p->valid.has(Stage::Trajectory)) return fail(RL_EINVAL, fn + ": no trajectory stage since the plan's last run");
    const QueryView q = query_view(*query);
    if (int rc = check_query(kind, q, p->traj_R, p->N, p->closed)) return rc;
    if (reads_bounds(kind) && !p->valid.has(Stage::Bounds)) return fail(RL_EINVAL, fn + ": no bounds stage since the plan's last trajectory stage");
    return query_enqueue(p, kind, q, hip_stream);
}

// the checked prologue of every rl_plan_fetch_<name>
template <QueryKind kind, class Out>
int plan_fetch(rl_plan* p, const Out* out) {
    static_assert(sizeof(Out) == kKinds[(int)kind].n_fields * sizeof(void*), "out is the kind's results struct");
    const KindInfo& k = kind_info(kind);
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (!out) return fail(RL_EINVAL, std::string("rl_plan_fetch_") + k.name + ": out is NULL");
    if (!p->valid.has(stage_of(kind))) return fail(RL_EINVAL, k.fetch_none);
    return query_fetch(p, kind, out);
}

}  // namespace

extern "C" {

// The preparation kernel packs the min-curvature rows and sums their lengths, then the
// min-time kernel evaluates them at max_outer_iters = 0, as rl_lap_eval launches it.
int rl_plan_lap(rl_plan* p, void* hip_stream) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (!(p->modes & RL_MODE_MINCURV)) return fail(RL_EINVAL, "rl_plan_lap: the plan has no RL_MODE_MINCURV");
    if (p->N == 0) return fail(RL_EINVAL, "rl_plan_lap: N == 0 (no path)");
    if (!p->valid.has(Stage::Run)) return fail(RL_EINVAL, "rl_plan_lap: the plan has not run");
    HIPCHK(hipSetDevice(p->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->run_stream();
    p->valid.invalidate(Stage::Lap);
    ++p->lap_epoch;                                    // the stage's rows are written again
    if (int rc = lap_alloc(p)) return rc;
    if (!p->ev_lap_mid) HIPCHK(hipEventCreate(&p->ev_lap_mid));
    if (int rc = stage_begin(p, Stage::Lap, st)) return rc;
    rl::PrepParams q{};
    q.x = p->mb[0].x;
    q.y = p->mb[0].y;
    q.centre = p->d_lap_center;
    q.L_out = p->d_Lmc;
    q.cfg_src = p->d_cfg;
    q.cfg_dst = p->d_cfg_lap;
    q.N = p->N; q.B = p->B; q.closed = p->closed; q.ncfg = p->ncfg;
    hipError_t e = rl::launch_path_prep(q, st);
    if (e != hipSuccess) return fail(RL_EHIP, std::string("path prep launch: ") + hipGetErrorString(e));
    HIPCHK(hipEventRecord(p->ev_lap_mid, st));
    // rl_lap_eval's launch: per-instance centres and lengths, empty rings, no seeds, no
    // completion flags, no precomputed corridor
    const ModeBufs& lb = p->lapb;
    rl::KParams kp{};
    kp.center = p->d_lap_center;
    kp.center_stride = (int64_t)2 * (int64_t)p->N;
    kp.Ls = p->d_Lmc;
    DevRing none;                                      // (valid addresses, never read: M = 0)
    none.vtx = p->ring.vtx; none.rec = p->ring.rec; none.flag = p->ring.flag; none.blk = p->ring.blk;
    none.fill(kp.ring, 0, 0);
    kp.cfg = p->d_cfg_lap;
    set_bufs(kp, lb);
    kp.N = p->N; kp.ncfg = p->ncfg; kp.B = p->B; kp.closed = p->closed;
    kp.shape_B = p->shape_batch();
    kp.L = p->L;
    e = p->stream ? rl::launch_stream(kp, lb.sb, true, st) : rl::launch_optimize(kp, true, st);
    if (e != hipSuccess) return fail(RL_EHIP, std::string("lap evaluation launch: ") + hipGetErrorString(e));
    return stage_end(p, Stage::Lap, st);
}

int rl_plan_fetch_lap(rl_plan* p, rl_out* out, double* path_len) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (!p->valid.has(Stage::Lap)) return fail(RL_EINVAL, "rl_plan_fetch_lap: no lap stage since the plan's last run");
    std::vector<CopyJob> jobs;
    field_jobs(out, p->lapb, {(size_t)p->B, (size_t)p->N, 0, 1}, true, true, jobs);
    add_job(jobs, path_len, p->d_Lmc, (size_t)p->B * 8);
    return stage_fetch(p, Stage::Lap, jobs);
}

int rl_plan_select(rl_plan* p, const rl_select* sel, void* hip_stream) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    int gs = 0;
    if (int rc = check_select(sel, p->B, p->N, p->modes, &gs)) return rc;
    if (!p->valid.has(Stage::Run)) return fail(RL_EINVAL, "rl_plan_select: the plan has not run");
    return select_impl(p, sel, gs, false, hip_stream);
}

int rl_plan_select_scored(rl_plan* p, const rl_select* sel, int32_t score, void* hip_stream) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (score != RL_SCORE_DEFAULT && score != RL_SCORE_LAP) return fail(RL_EINVAL, "select: unknown score");
    int gs = 0;
    if (int rc = check_select(sel, p->B, p->N, p->modes, &gs)) return rc;
    if (!p->valid.has(Stage::Run)) return fail(RL_EINVAL, "rl_plan_select: the plan has not run");
    const bool by_lap = score == RL_SCORE_LAP && sel->mode == RL_MODE_MINCURV;
    if (by_lap && !p->valid.has(Stage::Lap))
        if (int rc = rl_plan_lap(p, hip_stream)) return rc;
    return select_impl(p, sel, gs, by_lap, hip_stream);
}

int rl_plan_fetch_selected(rl_plan* p, int32_t* index, double* score, double* all_scores, rl_out* out) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (!index || !score) return fail(RL_EINVAL, "rl_plan_fetch_selected: index / score is NULL");
    if (!p->valid.has(Stage::Select)) return fail(RL_EINVAL, "rl_plan_fetch_selected: no selection since the plan's last run");
    std::vector<CopyJob> jobs;
    sel_jobs(p, index, score, all_scores, out, jobs);
    return stage_fetch(p, Stage::Select, jobs);
}

// One launch of rl_trajectory_kernel over the rows in force: the min-time optimiser's, or the
// min-curvature optimiser's x, y with the lap stage's heading, kappa, v, ax and lengths.
int rl_plan_trajectory(rl_plan* p, int32_t mode, int32_t rows, double dt, int32_t M_cap, void* hip_stream) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (mode != RL_MODE_MINCURV && mode != RL_MODE_MINTIME)
        return fail(RL_EINVAL, "trajectory: mode must be exactly one of RL_MODE_MINCURV, RL_MODE_MINTIME");
    if (!(p->modes & mode)) return fail(RL_EINVAL, "trajectory: mode is not among the plan's modes");
    if (int rc = check_traj(dt, M_cap)) return rc;
    if (p->N == 0) return fail(RL_EINVAL, "trajectory: N == 0 (no row)");
    if (rows != RL_TRAJ_ALL && rows != RL_TRAJ_SELECTED) return fail(RL_EINVAL, "trajectory: unknown rows");
    if (!p->valid.has(Stage::Run)) return fail(RL_EINVAL, "rl_plan_trajectory: the plan has not run");
    const bool selected = rows == RL_TRAJ_SELECTED;
    if (selected && (!p->valid.has(Stage::Select) || p->sel_mode != mode))
        return fail(RL_EINVAL, "rl_plan_trajectory: no selection of this mode since the plan's last run");
    const bool mc = mode == RL_MODE_MINCURV;
    p->valid.invalidate(Stage::Trajectory);            // and every stage that reads the one before this one
    if (mc && !p->valid.has(Stage::Lap))
        if (int rc = rl_plan_lap(p, hip_stream)) return rc;
    HIPCHK(hipSetDevice(p->device));
    const int R = selected ? p->sel_G * p->sel_k : p->B;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->run_stream();
    if (int rc = traj_alloc(p, R, M_cap)) return rc;
    if (int rc = stage_begin(p, Stage::Trajectory, st, (mc ? sbit(Stage::Lap) : 0) | (selected ? sbit(Stage::Select) : 0))) return rc;
    const ModeBufs& mb = p->mb[mc ? 0 : 1];
    const ModeBufs& src = mc ? p->lapb : mb;
    rl::TrajParams q{};
    q.x = mb.x; q.y = mb.y;
    q.heading = src.heading; q.kappa = src.kappa; q.v = src.v; q.ax = src.ax;
    q.Ls = mc ? p->d_Lmc : p->d_Ls;
    q.L = p->L;
    q.index = selected ? p->d_index : nullptr;
    for (int c = 0; c < TRAJ_COLS; ++c) q.out[c] = p->traj_col[c];
    q.stamps = p->traj_stamps;
    q.T = p->traj_T;
    q.count = p->traj_count;
    q.dt = dt;
    q.N = p->N; q.B = p->B; q.R = R; q.closed = p->closed; q.M_cap = M_cap;
    const hipError_t e = rl::launch_trajectory(q, st);
    if (e != hipSuccess) return fail(RL_EHIP, std::string("trajectory launch: ") + hipGetErrorString(e));
    p->traj_R = R;
    p->traj_M = M_cap;
    p->traj_q = q;                                     // what the horizon stage reads
    p->traj_mode = mode;
    p->traj_sel_epoch = p->sel_epoch;
    p->traj_lap_epoch = p->lap_epoch;
    return stage_end(p, Stage::Trajectory, st);
}

int rl_plan_fetch_trajectory(rl_plan* p, rl_traj* out) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (!out) return fail(RL_EINVAL, "rl_plan_fetch_trajectory: out is NULL");
    if (!p->valid.has(Stage::Trajectory)) return fail(RL_EINVAL, "rl_plan_fetch_trajectory: no trajectory stage since the plan's last run");
    std::vector<CopyJob> jobs;
    traj_jobs(p, out, jobs);
    return stage_fetch(p, Stage::Trajectory, jobs);
}

// the pose-query stages: plan_stage and plan_fetch with the kind
int rl_plan_horizon(rl_plan* p, const rl_hzn_query* query, void* hip_stream) { return plan_stage<QueryKind::Horizon>(p, query, hip_stream); }
int rl_plan_fetch_horizon(rl_plan* p, rl_hzn* out) { return plan_fetch<QueryKind::Horizon>(p, out); }
int rl_plan_rejoin(rl_plan* p, const rl_rjn_query* query, void* hip_stream) { return plan_stage<QueryKind::Rejoin>(p, query, hip_stream); }
int rl_plan_fetch_rejoin(rl_plan* p, rl_rjn* out) { return plan_fetch<QueryKind::Rejoin>(p, out); }
int rl_plan_stop(rl_plan* p, const rl_stp_query* query, void* hip_stream) { return plan_stage<QueryKind::Stop>(p, query, hip_stream); }
int rl_plan_fetch_stop(rl_plan* p, rl_stp* out) { return plan_fetch<QueryKind::Stop>(p, out); }
int rl_plan_retime(rl_plan* p, const rl_rtm_query* query, void* hip_stream) { return plan_stage<QueryKind::Retime>(p, query, hip_stream); }
int rl_plan_fetch_retime(rl_plan* p, rl_rtm* out) { return plan_fetch<QueryKind::Retime>(p, out); }
int rl_plan_recover(rl_plan* p, const rl_rcv_query* query, void* hip_stream) { return plan_stage<QueryKind::Recover>(p, query, hip_stream); }
int rl_plan_fetch_recover(rl_plan* p, rl_rcv* out) { return plan_fetch<QueryKind::Recover>(p, out); }
int rl_plan_recover_fan(rl_plan* p, const rl_fan_query* query, void* hip_stream) { return plan_stage<QueryKind::Fan>(p, query, hip_stream); }
int rl_plan_fetch_recover_fan(rl_plan* p, rl_fan* out) { return plan_fetch<QueryKind::Fan>(p, out); }

// One launch of rl_bounds_kernel over the rows the last trajectory stage read: its x, y and
// index, the plan's resident rings.  Buffers of its own: every other stage stays as it is.
int rl_plan_bounds(rl_plan* p, const rl_bnd_query* query, void* hip_stream) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (!query) return fail(RL_EINVAL, "bounds: the query is NULL");
    if (!std::isfinite(query->veh_width) || !std::isfinite(query->margin))
        return fail(RL_EINVAL, "bounds: veh_width or margin is not finite");
    if (!p->valid.has(Stage::Trajectory)) return fail(RL_EINVAL, "rl_plan_bounds: no trajectory stage since the plan's last run");
    if (int rc = traj_current(p, "rl_plan_bounds")) return rc;
    HIPCHK(hipSetDevice(p->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->run_stream();
    p->valid.invalidate(Stage::Bounds);                // (and what read the stage before this one)
    if (int rc = bounds_alloc(p, p->traj_R)) return rc;
    unsigned readers = 0;                              // (valid or not, they may still read the rows, on another stream)
    for (int s = 0; s < N_STAGES; ++s)
        if (stage_reads((Stage)s, Stage::Bounds)) readers |= 1u << s;
    if (int rc = stage_begin(p, Stage::Bounds, st, readers)) return rc;
    const TrajParams& t = p->traj_q;
    rl::BndParams b{};
    b.x = t.x; b.y = t.y;
    b.index = t.index;
    p->ring.fill(b.ring, p->Ei, p->Eo);
    b.guard = query->veh_width * 0.5 + query->margin;  // ref:706, as rl_corridor forms it
    b.lo = p->bnd[0]; b.hi = p->bnd[1]; b.nx = p->bnd[2]; b.ny = p->bnd[3];
    b.N = t.N; b.B = t.B; b.R = t.R; b.closed = t.closed;
    const hipError_t e = rl::launch_bounds(b, st);
    if (e != hipSuccess) return fail(RL_EHIP, std::string("bounds launch: ") + hipGetErrorString(e));
    p->bnd_R = t.R;
    return stage_end(p, Stage::Bounds, st);
}

int rl_plan_fetch_bounds(rl_plan* p, rl_bnd* out) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (!out) return fail(RL_EINVAL, "rl_plan_fetch_bounds: out is NULL");
    if (!p->valid.has(Stage::Bounds))
        return fail(RL_EINVAL, "rl_plan_fetch_bounds: no bounds stage since the plan's last run or trajectory stage");
    double* const dst[4] = {out->lo, out->hi, out->nx, out->ny};
    std::vector<CopyJob> jobs;
    for (int c = 0; c < 4; ++c) add_job(jobs, dst[c], p->bnd[c], (size_t)p->bnd_R * (size_t)p->N * 8);
    return stage_fetch(p, Stage::Bounds, jobs);
}

// One launch of rl_horizon_bounds_kernel on what the last horizon stage left in its results'
// block and the bounds stage's rows: no upload.
int rl_plan_horizon_bounds(rl_plan* p, void* hip_stream) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (!p->valid.has(Stage::Horizon) || !p->valid.has(Stage::Bounds))
        return fail(RL_EINVAL, "rl_plan_horizon_bounds: no horizon stage and bounds stage since the plan's last trajectory stage");
    HIPCHK(hipSetDevice(p->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->run_stream();
    const QueryStage& s = p->stage(QueryKind::Horizon);
    p->valid.invalidate(Stage::HorizonBounds);
    if (int rc = horizon_bounds_alloc(p, (size_t)s.Q, (size_t)s.M)) return rc;
    if (int rc = stage_begin(p, Stage::HorizonBounds, st)) return rc;
    // the horizon stage's launch again, as query_enqueue made it
    rl_rjn_query q{};
    q.Q = s.Q; q.M_cap = s.M; q.dt = s.dt;
    rl::HznBndParams h{};
    h.hz = query_pointers(q, query_layout_of(QueryKind::Horizon, (size_t)s.Q, (size_t)s.M, 0), s.in, s.out).hz;
    h.hz.src = p->traj_q;
    h.lo = p->bnd[0]; h.hi = p->bnd[1];
    h.tlo = p->hb[0]; h.thi = p->hb[1]; h.lo0 = p->hb[2]; h.hi0 = p->hb[3];
    const hipError_t e = rl::launch_horizon_bounds(h, st);
    if (e != hipSuccess) return fail(RL_EHIP, std::string("horizon bounds launch: ") + hipGetErrorString(e));
    p->hb_Q = s.Q;
    p->hb_M = s.M;
    return stage_end(p, Stage::HorizonBounds, st);
}

int rl_plan_fetch_horizon_bounds(rl_plan* p, rl_hzn_bnd* out) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (!out) return fail(RL_EINVAL, "rl_plan_fetch_horizon_bounds: out is NULL");
    if (!p->valid.has(Stage::HorizonBounds))
        return fail(RL_EINVAL, "rl_plan_fetch_horizon_bounds: no rl_plan_horizon_bounds since the plan's last run or stage it reads");
    const size_t Q = (size_t)p->hb_Q, M = (size_t)p->hb_M;
    double* const dst[4] = {out->lo, out->hi, out->lo0, out->hi0};
    std::vector<CopyJob> jobs;
    for (int c = 0; c < 4; ++c) add_job(jobs, dst[c], p->hb[c], (c < 2 ? Q * M : Q) * 8);
    return stage_fetch(p, Stage::HorizonBounds, jobs);
}

// One launch of rl_rollout_kernel on the last trajectory stage's rows and the bounds stage's rows
// of the same, then rl_rank_kernel on the costs (upload_launch, as the pose-query kinds).
int rl_plan_rollouts(rl_plan* p, const rl_rll_query* query, void* hip_stream) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (!query) return fail(RL_EINVAL, "rollouts: the query or its xy is NULL");
    if (!p->valid.has(Stage::Trajectory)) return fail(RL_EINVAL, "rl_plan_rollouts: no trajectory stage since the plan's last run");
    int gs = 0;
    if (int rc = check_rollouts(*query, p->traj_R, &gs)) return rc;
    if (!p->valid.has(Stage::Bounds)) return fail(RL_EINVAL, "rl_plan_rollouts: no bounds stage since the plan's last trajectory stage");
    if (int rc = traj_current(p, "rl_plan_rollouts")) return rc;
    HIPCHK(hipSetDevice(p->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->run_stream();
    QueryStage& s = p->rll;
    const RllLayout L = rll_layout((size_t)query->Q, (size_t)query->T, (size_t)(query->Q / gs) * (size_t)query->k,
                                   query->v != nullptr, query->row != nullptr, query->seg_hint != nullptr);
    const int rc = upload_launch(
        p, Stage::Rollouts, s, L, 0, st, [&](char* pin) { rll_pack(*query, L, pin); },
        [&] { return rll_launch(L, *query, gs, p->traj_q, p->bnd[0], p->bnd[1], s.in, s.out, st); });
    if (rc) return rc;
    s.Q = query->Q;
    s.M = query->T;
    p->rll_R = (int)L.R;
    return RL_OK;
}

int rl_plan_fetch_rollouts(rl_plan* p, rl_rll* out) {
    if (!p) return fail(RL_EINVAL, "plan is NULL");
    if (!out) return fail(RL_EINVAL, "rl_plan_fetch_rollouts: results is NULL");
    if (!p->valid.has(Stage::Rollouts))
        return fail(RL_EINVAL, "rl_plan_fetch_rollouts: no rollouts stage since the plan's last run, trajectory or bounds stage");
    HIPCHK(hipSetDevice(p->device));
    QueryStage& s = p->rll;
    hipStream_t st = p->run_stream();
    if (int rc = stage_wait(p, Stage::Rollouts, st)) return rc;   // (a later stage may have moved to another stream)
    const RllLayout L = rll_layout((size_t)s.Q, (size_t)s.M, (size_t)p->rll_R, false, false, false);
    const bool poses = rll_wants_poses(out);
    HIPCHK(hipMemcpyAsync(s.pin, s.out, poses ? L.out_bytes : L.head_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    rll_unpack(s.pin, L, out, poses);
    return RL_OK;
}

}  // extern "C"
