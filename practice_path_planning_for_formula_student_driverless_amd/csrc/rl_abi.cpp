// rl_abi.cpp — C-ABI implementation (include/rl_abi.h), part 1: the queries that need no
// plan, the cfg defaults, and the one-shot entry points that upload, run one kernel and
// download.  Plans are in rl_plan.cpp, their stages in rl_stages.cpp, rl_optimize and the
// plan cache in rl_cache.cpp.  The compute path is the gfx950 kernels; there is no CPU fallback.
#include "rl_host.h"

using namespace rl;

namespace {

// The B host rows in[6] (x, y, heading, kappa, v, ax: [B][N]) and their steps h [B] on the
// device, with the outputs of a trajectory stage of M_cap ticks over them, all from `mem`:
// *q is that launch.  fn names the entry point in the messages.
int rows_on_device(DevArena& mem, const std::string& fn, const double* const (&in)[6], const double* h, int32_t N,
                   int32_t B, int32_t closed, double dt, int32_t M_cap, rl::TrajParams* q) {
    const size_t R = (size_t)B, BN = R * (size_t)N;
    double* d_in[6];
    for (auto& d : d_in) d = mem.get<double>(BN);
    double* d_h = mem.get<double>(R);
    *q = rl::TrajParams{};
    for (auto& c : q->out) c = mem.get<double>(R * (size_t)M_cap);
    q->stamps = mem.get<double>(R * ((size_t)N + 1));
    q->T = mem.get<double>(R);
    q->count = mem.get<int32_t>(R);
    if (!mem.ok()) return fail(RL_ENOMEM, fn + ": hipMalloc failed");
    for (int c = 0; c < 6; ++c)
        if (BN && hipMemcpy(d_in[c], in[c], BN * 8, hipMemcpyHostToDevice) != hipSuccess) return fail(RL_EHIP, fn + ": upload");
    if (hipMemcpy(d_h, h, R * 8, hipMemcpyHostToDevice) != hipSuccess) return fail(RL_EHIP, fn + ": upload");
    q->x = d_in[0]; q->y = d_in[1]; q->heading = d_in[2]; q->kappa = d_in[3]; q->v = d_in[4]; q->ax = d_in[5];
    q->h = d_h;
    q->dt = dt;
    q->N = N; q->B = B; q->R = B; q->closed = closed ? 1 : 0; q->M_cap = M_cap;
    return RL_OK;
}

// every pose-query stage's one-shot rl_<name> (arguments checked, the device selected; out: the
// kind's results struct; bnd: the rows' bounds lo, hi, nx, ny [B][N] on the host, for a kind that
// reads them): the trajectory kernel for the stamps of the host rows (one tick per row, not
// downloaded), then the kind's kernel on them; `row` counts the B given rows
int query_rows(const std::string& fn, const double* const (&in)[6], const double* h, int32_t N, int32_t B, int32_t closed,
               QueryKind kind, const QueryView& q, const void* out, const double* const (&bnd)[4]) {
    const bool bounds = reads_bounds(kind);
    DevArena mem;
    rl::TrajParams t;
    if (int rc = rows_on_device(mem, fn, in, h, N, B, closed, q.rj.dt, 1, &t)) return rc;
    const QueryLayout L = query_layout_of(kind, q);
    double* d_bnd[4] = {};
    char* d_scratch = L.scratch_bytes ? mem.get<char>(L.scratch_bytes) : nullptr;
    if (bounds)
        for (auto& d : d_bnd) d = mem.get<double>((size_t)B * (size_t)N);
    char* d_qry = mem.get<char>(L.in_bytes);
    char* d_res = mem.get<char>(L.out_bytes);
    if (!mem.ok()) return fail(RL_ENOMEM, fn + ": hipMalloc failed");
    std::vector<char> block(std::max(L.in_bytes, L.out_bytes));
    query_pack(q, L, block.data());
    if (hipMemcpy(d_qry, block.data(), L.in_bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(RL_EHIP, fn + ": upload");
    for (int c = 0; bounds && c < 4; ++c)
        if (hipMemcpy(d_bnd[c], bnd[c], (size_t)B * (size_t)N * 8, hipMemcpyHostToDevice) != hipSuccess)
            return fail(RL_EHIP, fn + ": upload");
    if (rl::launch_trajectory(t, nullptr) != hipSuccess) return fail(RL_EHIP, fn + ": trajectory kernel");
    const hipError_t e = query_launch(L, q, t, d_qry, d_res, {d_bnd[0], d_bnd[1], d_bnd[2], d_bnd[3]}, d_scratch, nullptr);
    if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(RL_EHIP, fn + ": kernel");
    if (hipMemcpy(block.data(), d_res, query_wants_nodes(kind, out) ? L.out_bytes : L.head_bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(RL_EHIP, fn + ": download");
    query_unpack(block.data(), L, out);
    return RL_OK;
}

// the checked prologue of every rl_<name>: rows = x, y, heading, kappa, v, ax, h and, for a kind
// that reads the bounds, lo, hi, nx, ny
template <QueryKind kind, class Query, class Out>
int one_shot(const double* const (&rows)[11], int32_t N, int32_t B, int32_t closed, const Query* query, int32_t device, Out* out) {
    static_assert(sizeof(Out) == kKinds[(int)kind].n_fields * sizeof(void*), "out is the kind's results struct");
    const KindInfo& k = kind_info(kind);
    const std::string fn = std::string("rl_") + k.name;
    bool null = !query || !out;
    for (int c = 0; c < (reads_bounds(kind) ? 11 : 7); ++c) null = null || !rows[c];
    if (null)
        return fail(RL_EINVAL, fn + (reads_bounds(kind) ? ": an input row, h, a bounds row, the query or out is NULL"
                                                    : ": an input row, h, the query or out is NULL"));
    if (B < 1 || N < 0) return fail(RL_EINVAL, fn + ": B < 1 or N < 0");
    if (N > rl::RL_STREAM_MAX_N) return fail(RL_ETOOBIG, fn + ": N exceeds 1048576");
    const QueryView q = query_view(*query);
    if (int rc = check_query(kind, q, B, N, closed ? 1 : 0)) return rc;
    if (int rc = select_device(device)) return rc;
    return query_rows(fn, {rows[0], rows[1], rows[2], rows[3], rows[4], rows[5]}, rows[6], N, B, closed, kind, q, out,
                      {rows[7], rows[8], rows[9], rows[10]});
}

}  // namespace

extern "C" {

const char* rl_last_error(void) { return g_err.c_str(); }
int rl_abi_version(void) { return RL_ABI_VERSION; }
int rl_abi_minor(void) { return RL_ABI_MINOR; }
int rl_abi_features(void) {
    return RL_FEATURE_TRAJECTORY | RL_FEATURE_HORIZON | RL_FEATURE_REJOIN | RL_FEATURE_STOP | RL_FEATURE_BOUNDS |
           RL_FEATURE_RETIME | RL_FEATURE_RECOVER | RL_FEATURE_FAN | RL_FEATURE_ROLLOUT;
}

int rl_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// samples per lane of the register-resident kernel (4 or 8), 1 for the streaming
// kernel, RL_ETOOBIG beyond it
int rl_kernel_variant(int32_t N) {
    if (N > rl::RL_STREAM_MAX_N) return RL_ETOOBIG;
    if (use_stream(N)) return 1;
    const int k = rl::fit_shape(rl::THR_SHAPES, N).K;
    return k < 0 ? RL_ETOOBIG : k;
}

// (K, T) the library launches for N samples, a batch of B and `mode` (one of
// RL_MODE_MINCURV / RL_MODE_MINTIME) on the calling thread's current device
int rl_kernel_shape(int32_t N, int32_t B, int32_t mode, int32_t* K, int32_t* T) {
    if (!K || !T || B < 1 || (mode != RL_MODE_MINCURV && mode != RL_MODE_MINTIME))
        return fail(RL_EINVAL, "rl_kernel_shape: bad argument");
    if (N < 1 || N > rl::RL_STREAM_MAX_N) return fail(RL_ETOOBIG, "rl_kernel_shape: N out of range");
    if (use_stream(N)) { *K = 0; *T = rl::stream_threads(); return RL_OK; }   // streaming kernel (samples strided)
    int dev = 0;
    const int cus = (hipGetDevice(&dev) == hipSuccess) ? device_cus(dev) : 256;
    const rl::Shape s = rl::pick_shape(N, B, mode == RL_MODE_MINTIME, cus);
    *K = s.K;
    *T = s.T;
    return RL_OK;
}

// cfg::Config defaults, ref:77-113
void rl_cfg_default(rl_cfg* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->veh_width_m = 1.0;
    c->safety_margin_m = 0.05;
    c->lambda_smooth = 1.6e-3;
    c->max_outer_iters = 14;
    c->max_inner_iters = 120;
    c->step_init = 0.65;
    c->step_min = 1e-6;
    c->armijo_c = 1e-5;
    c->kappa_eps = 1e-6;
    c->v_cap_mps = 27.0;
    c->mass_kg = 255.0;
    c->Cd = 0.30;
    c->A_front_m2 = 1.00;
    c->rho_air = 1.225;
    c->c_rr = 0.015;
    c->P_max_W = 80000.0;
    c->mu = 1.17;
    c->a_total_max = c->mu * 9.81;   // ref:102 (evaluated once)
    c->a_lat_max = 11.0;
    c->a_long_acc_cap = 8.0;
    c->a_long_brake_cap = 11.0;
    c->w_time_gain = 1.0;
    c->time_gamma_power = 2.0;
    c->time_weight_use_inv_v = 0;
    c->inv_v_gain = 0.1;
    c->max_vpass_iters = 6;
    c->use_total_ge_lat = 1;
}

void rl_cfg_set_mu(rl_cfg* c, double mu) {
    if (!c) return;
    c->mu = mu;
    c->a_total_max = mu * 9.81;
}

// edges::ringEdges ref:251-255 / edges::polylineEdges ref:256-260
int rl_ring_segments(const double* ring_xy, int32_t n, int32_t closed, double* seg_out) {
    if (n < 0 || (n > 0 && (!ring_xy || !seg_out))) return fail(RL_EINVAL, "rl_ring_segments: bad argument");
    if (closed) {
        for (int i = 0; i < n; ++i) {
            int j = (i + 1) % n;
            seg_out[4 * i] = ring_xy[2 * i];
            seg_out[4 * i + 1] = ring_xy[2 * i + 1];
            seg_out[4 * i + 2] = ring_xy[2 * j];
            seg_out[4 * i + 3] = ring_xy[2 * j + 1];
        }
        return n;
    }
    if (n < 2) return 0;
    for (int i = 0; i + 1 < n; ++i) {
        seg_out[4 * i] = ring_xy[2 * i];
        seg_out[4 * i + 1] = ring_xy[2 * i + 1];
        seg_out[4 * i + 2] = ring_xy[2 * i + 2];
        seg_out[4 * i + 3] = ring_xy[2 * i + 3];
    }
    return n - 1;
}

double rl_seed_value(uint64_t seed, int32_t i, double sigma) { return rl::seed_value(seed, i, sigma); }

// pipeline::compute_geom_and_save rows (ref:1295-1335) on the device
int rl_corridor(const rl_problem* prob, const rl_cfg* cfg, int32_t device, double* lo, double* hi) {
    if (!prob || !cfg || !lo || !hi) return fail(RL_EINVAL, "rl_corridor: NULL argument");
    if (prob->N < 0 || (prob->N > 0 && !prob->center_xy)) return fail(RL_EINVAL, "rl_corridor: bad centre");
    if (prob->Ei < 0 || prob->Eo < 0 || (prob->Ei > 0 && !prob->inner_seg) || (prob->Eo > 0 && !prob->outer_seg))
        return fail(RL_EINVAL, "rl_corridor: bad segments");
    if (int rc = select_device(device)) return rc;
    const int N = prob->N;
    if (N == 0) return RL_OK;
    const RingHost rh[2] = {make_ring(prob->inner_seg, prob->Ei), make_ring(prob->outer_seg, prob->Eo)};
    DevArena mem;
    DevRing ring;
    double* d_c = mem.get<double>(2 * (size_t)N);
    double* d_out = mem.get<double>(2 * (size_t)N);
    if (!ring.alloc(mem, rh)) return fail(RL_ENOMEM, "rl_corridor: hipMalloc failed");
    rl::CorrParams c{};
    c.center = d_c;
    c.N = N;
    c.closed = prob->closed ? 1 : 0;
    ring.fill(c.ring, rh[0].E, rh[1].E);
    c.guard = prob->veh_width * 0.5 + cfg->safety_margin_m;     // ref:706
    c.lo = d_out;
    c.hi = d_out + N;
    if (hipMemcpy(d_c, prob->center_xy, 2 * (size_t)N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        !ring.upload(rh, nullptr))
        return fail(RL_EHIP, "rl_corridor: upload");
    if (rl::launch_corridor(c, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(RL_EHIP, "rl_corridor: kernel");
    if (hipMemcpy(lo, d_out, (size_t)N * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(hi, d_out + N, (size_t)N * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(RL_EHIP, "rl_corridor: download");
    return RL_OK;
}

// the bounds stage's kernel (rl_bounds.hip) on B host rows: the rings go up once for all of them
int rl_bounds(const rl_problem* prob, const double* x, const double* y, int32_t B, double veh_width, double margin,
              int32_t device, rl_bnd* out) {
    if (!prob || !x || !y || !out) return fail(RL_EINVAL, "rl_bounds: prob, x, y or out is NULL");
    if (B < 1 || prob->N < 0) return fail(RL_EINVAL, "rl_bounds: B < 1 or N < 0");
    if (prob->Ei < 0 || prob->Eo < 0 || (prob->Ei > 0 && !prob->inner_seg) || (prob->Eo > 0 && !prob->outer_seg))
        return fail(RL_EINVAL, "rl_bounds: bad segments");
    if (!std::isfinite(veh_width) || !std::isfinite(margin)) return fail(RL_EINVAL, "rl_bounds: veh_width or margin is not finite");
    if (prob->N > rl::RL_STREAM_MAX_N) return fail(RL_ETOOBIG, "rl_bounds: N exceeds 1048576");
    if (int rc = select_device(device)) return rc;
    const int N = prob->N;
    if (N == 0) return RL_OK;
    const size_t BN = (size_t)B * (size_t)N;
    const RingHost rh[2] = {make_ring(prob->inner_seg, prob->Ei), make_ring(prob->outer_seg, prob->Eo)};
    DevArena mem;
    DevRing ring;
    double* d_xy = mem.get<double>(2 * BN);
    double* d_out = mem.get<double>(4 * BN);
    if (!ring.alloc(mem, rh)) return fail(RL_ENOMEM, "rl_bounds: hipMalloc failed");
    rl::BndParams b{};
    b.x = d_xy; b.y = d_xy + BN;
    ring.fill(b.ring, rh[0].E, rh[1].E);
    b.guard = veh_width * 0.5 + margin;                          // ref:706
    b.lo = d_out; b.hi = d_out + BN; b.nx = d_out + 2 * BN; b.ny = d_out + 3 * BN;
    b.N = N; b.B = B; b.R = B; b.closed = prob->closed ? 1 : 0;
    if (hipMemcpy(d_xy, x, BN * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_xy + BN, y, BN * sizeof(double), hipMemcpyHostToDevice) != hipSuccess || !ring.upload(rh, nullptr))
        return fail(RL_EHIP, "rl_bounds: upload");
    if (rl::launch_bounds(b, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(RL_EHIP, "rl_bounds: kernel");
    double* const dst[4] = {out->lo, out->hi, out->nx, out->ny};
    for (int c = 0; c < 4; ++c)
        if (dst[c] && hipMemcpy(dst[c], d_out + (size_t)c * BN, BN * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(RL_EHIP, "rl_bounds: download");
    return RL_OK;
}

int rl_geom(const rl_geom_problem* gp, const rl_cfg* cfg, int32_t device, double* rows, float* kernel_ms) {
    if (!gp || !cfg || !rows) return fail(RL_EINVAL, "rl_geom: NULL argument");
    if (gp->Kmax < 0 || gp->denomN == 0) return fail(RL_EINVAL, "rl_geom: Kmax < 0 or denomN == 0");
    if (gp->spx.n != gp->spy.n || gp->spx.n < 0) return fail(RL_EINVAL, "rl_geom: spline sizes differ");
    if (gp->Ei < 0 || gp->Eo < 0 || (gp->Ei > 0 && !gp->inner_seg) || (gp->Eo > 0 && !gp->outer_seg))
        return fail(RL_EINVAL, "rl_geom: bad segments");
    const int nk = gp->spx.n;
    const rl_spline* sp[2] = {&gp->spx, &gp->spy};
    for (int a = 0; a < 2; ++a)
        if (nk > 0 && (!sp[a]->s || !sp[a]->a || !sp[a]->b || !sp[a]->c || !sp[a]->d))
            return fail(RL_EINVAL, "rl_geom: NULL spline array");
    if (int rc = select_device(device)) return rc;
    const int nrows = gp->Kmax + (gp->emit_closed_duplicate ? 1 : 0);
    if (gp->Kmax == 0) {                      // no rows computed: the duplicate is (L, 0, ..., 0)
        if (nrows) { std::memset(rows, 0, sizeof(double) * RL_GEOM_COLS); rows[0] = gp->L; }
        if (kernel_ms) *kernel_ms = 0.0f;
        return nrows;
    }
    const RingHost rh[2] = {make_ring(gp->inner_seg, gp->Ei), make_ring(gp->outer_seg, gp->Eo)};
    std::vector<double> kn((size_t)10 * std::max(nk, 1), 0.0);
    for (int a = 0; a < 2; ++a) {
        const double* arr[5] = {sp[a]->s, sp[a]->a, sp[a]->b, sp[a]->c, sp[a]->d};
        for (int j = 0; j < 5; ++j)
            if (nk) std::memcpy(&kn[(size_t)(5 * a + j) * nk], arr[j], sizeof(double) * nk);
    }
    DevArena mem;                             // (freed after `finish` has drained the stream)
    DevRing ring;
    double* d_kn = mem.get<double>(kn.size());
    double* d_rows = mem.get<double>((size_t)nrows * RL_GEOM_COLS);
    if (!ring.alloc(mem, rh)) return fail(RL_ENOMEM, "rl_geom: hipMalloc failed");
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return fail(RL_EHIP, "rl_geom: stream");
    auto finish = [&](int code) {
        if (e0) hipEventDestroy(e0);
        if (e1) hipEventDestroy(e1);
        hipStreamSynchronize(st);
        hipStreamDestroy(st);
        return code;
    };
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return finish(fail(RL_EHIP, "rl_geom: events"));
    if (hipMemcpyAsync(d_kn, kn.data(), kn.size() * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
        return finish(fail(RL_EHIP, "rl_geom: upload knots"));
    if (!ring.upload(rh, st)) return finish(fail(RL_EHIP, "rl_geom: upload rings"));
    rl::GeomParams g{};
    ring.fill(g.ring, rh[0].E, rh[1].E);
    g.kx = d_kn;
    g.ky = d_kn + 5 * (size_t)nk;
    g.nk = nk;
    g.Kmax = gp->Kmax;
    g.denomN = gp->denomN;
    g.emit_dup = gp->emit_closed_duplicate ? 1 : 0;
    g.s0 = gp->s0;
    g.L = gp->L;
    g.kappa_eps = cfg->kappa_eps;
    g.a_lat_max = cfg->a_lat_max;
    g.v_cap = cfg->v_cap_mps;
    g.rows = d_rows;
    if (hipEventRecord(e0, st) != hipSuccess) return finish(fail(RL_EHIP, "rl_geom: event"));
    if (rl::launch_geom(g, st) != hipSuccess) return finish(fail(RL_EHIP, "rl_geom: kernel launch"));
    if (hipEventRecord(e1, st) != hipSuccess) return finish(fail(RL_EHIP, "rl_geom: event"));
    if (hipMemcpyAsync(rows, d_rows, (size_t)nrows * RL_GEOM_COLS * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return finish(fail(RL_EHIP, "rl_geom: download"));
    if (kernel_ms) {
        float ms = 0.0f;
        hipEventElapsedTime(&ms, e0, e1);
        *kernel_ms = ms;
    }
    return finish(nrows);
}

// glibc "%.9f" CSV rows of a host table, formatted on the device (rl_format.hip)
int rl_format_csv(const double* table, int64_t rows, int32_t cols, int32_t device, char* out, int64_t out_cap,
                  int64_t* out_len, int64_t* row_offsets) {
    if (!out_len || rows < 0 || cols < 1 || (rows > 0 && !table) || (out_cap > 0 && !out))
        return fail(RL_EINVAL, "rl_format_csv: bad argument");
    *out_len = 0;
    if (rows == 0) {
        if (row_offsets) row_offsets[0] = 0;
        return RL_OK;
    }
    if (rows > (int64_t)1 << 31) return fail(RL_ETOOBIG, "rl_format_csv: more than 2^31 rows");
    if (int rc = select_device(device)) return rc;
    const uint64_t cap = (uint64_t)rows * (uint64_t)cols * 22;
    DevArena mem;                             // (freed after `done` has drained the stream)
    hipStream_t st = nullptr;
    auto done = [&](int code) {
        if (st) { hipStreamSynchronize(st); hipStreamDestroy(st); }
        return code;
    };
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return done(fail(RL_EHIP, "stream"));
    double* d_tab = mem.get<double>((size_t)rows * cols);
    char* d_out = mem.get<char>(cap);
    uint64_t* d_offs = mem.get<uint64_t>((size_t)(rows + 1));
    if (!mem.ok()) return done(fail(RL_ENOMEM, "rl_format_csv: hipMalloc failed"));
    if (hipMemcpyAsync(d_tab, table, (size_t)rows * cols * 8, hipMemcpyHostToDevice, st) != hipSuccess)
        return done(fail(RL_EHIP, "rl_format_csv: upload"));
    uint64_t total = 0;
    const int rc = rl::format_rows(d_tab, rows, cols, d_out, cap, d_offs, &total, st);
    if (rc == -1) return done(fail(RL_ETOOBIG, "rl_format_csv: a value with |x| >= 9.2e9"));
    if (rc != 0) return done(fail(RL_EHIP, "rl_format_csv: device formatting failed"));
    *out_len = (int64_t)total;
    if ((int64_t)total > out_cap) return done(fail(RL_ETOOBIG, "rl_format_csv: out_cap too small (see *out_len)"));
    if (hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (row_offsets && hipMemcpyAsync(row_offsets, d_offs, (size_t)(rows + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return done(fail(RL_EHIP, "rl_format_csv: download"));
    return done(RL_OK);
}

// the prep kernel alone on host paths (rl_lap_stage.hip)
int rl_path_lengths(const double* x, const double* y, int32_t N, int32_t B, int32_t closed, int32_t device,
                    double* L_out) {
    if (!x || !y || !L_out) return fail(RL_EINVAL, "rl_path_lengths: x / y / L_out is NULL");
    if (B < 1 || N < 0) return fail(RL_EINVAL, "rl_path_lengths: B < 1 or N < 0");
    if (N > rl::RL_STREAM_MAX_N) return fail(RL_ETOOBIG, "rl_path_lengths: N exceeds 1048576");
    if (int rc = select_device(device)) return rc;
    const size_t BN = (size_t)B * (size_t)N, bytes = BN * 8;
    DevArena mem;
    double* d_x = mem.get<double>(BN);
    double* d_y = mem.get<double>(BN);
    double* d_L = mem.get<double>((size_t)B);
    if (!mem.ok()) return fail(RL_ENOMEM, "rl_path_lengths: hipMalloc failed");
    if (bytes && (hipMemcpy(d_x, x, bytes, hipMemcpyHostToDevice) != hipSuccess ||
                  hipMemcpy(d_y, y, bytes, hipMemcpyHostToDevice) != hipSuccess))
        return fail(RL_EHIP, "rl_path_lengths: upload");
    rl::PrepParams q{};
    q.x = d_x;
    q.y = d_y;
    q.L_out = d_L;
    q.N = N; q.B = B; q.closed = closed ? 1 : 0;
    if (rl::launch_path_prep(q, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(RL_EHIP, "rl_path_lengths: kernel");
    if (hipMemcpy(L_out, d_L, (size_t)B * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(RL_EHIP, "rl_path_lengths: download");
    return RL_OK;
}

// the trajectory kernel alone on host rows (rl_trajectory.hip): output row b is row b
int rl_trajectory(const double* x, const double* y, const double* heading, const double* kappa, const double* v,
                  const double* ax, const double* h, int32_t N, int32_t B, int32_t closed, double dt, int32_t M_cap,
                  int32_t device, rl_traj* out) {
    if (!x || !y || !heading || !kappa || !v || !ax || !h || !out)
        return fail(RL_EINVAL, "rl_trajectory: an input row, h or out is NULL");
    if (B < 1 || N < 0) return fail(RL_EINVAL, "rl_trajectory: B < 1 or N < 0");
    if (int rc = check_traj(dt, M_cap)) return rc;
    if (N > rl::RL_STREAM_MAX_N) return fail(RL_ETOOBIG, "rl_trajectory: N exceeds 1048576");
    if (int rc = select_device(device)) return rc;
    DevArena mem;
    rl::TrajParams q;
    if (int rc = rows_on_device(mem, "rl_trajectory", {x, y, heading, kappa, v, ax}, h, N, B, closed, dt, M_cap, &q)) return rc;
    if (rl::launch_trajectory(q, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(RL_EHIP, "rl_trajectory: kernel");
    const size_t BM = (size_t)B * (size_t)M_cap;
    double* const dst[rl::TRAJ_COLS] = {out->s, out->x, out->y, out->heading, out->kappa, out->v, out->ax};
    std::vector<CopyJob> jobs;
    for (int c = 0; c < rl::TRAJ_COLS; ++c) add_job(jobs, dst[c], q.out[c], BM * 8);
    add_job(jobs, out->stamps, q.stamps, (size_t)B * ((size_t)N + 1) * 8);
    add_job(jobs, out->T, q.T, (size_t)B * 8);
    add_job(jobs, out->count, q.count, (size_t)B * 4);
    for (const CopyJob& j : jobs)
        if (hipMemcpy(j.dst, j.src, j.bytes, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(RL_EHIP, "rl_trajectory: download");
    return RL_OK;
}

// the pose-query stages on host rows: one_shot with the kind
int rl_horizon(const double* x, const double* y, const double* heading, const double* kappa, const double* v,
               const double* ax, const double* h, int32_t N, int32_t B, int32_t closed, const rl_hzn_query* query,
               int32_t device, rl_hzn* out) {
    return one_shot<QueryKind::Horizon>({x, y, heading, kappa, v, ax, h, nullptr, nullptr, nullptr, nullptr}, N, B, closed, query, device, out);
}

int rl_rejoin(const double* x, const double* y, const double* heading, const double* kappa, const double* v,
              const double* ax, const double* h, int32_t N, int32_t B, int32_t closed, const rl_rjn_query* query,
              int32_t device, rl_rjn* out) {
    return one_shot<QueryKind::Rejoin>({x, y, heading, kappa, v, ax, h, nullptr, nullptr, nullptr, nullptr}, N, B, closed, query, device, out);
}

int rl_stop(const double* x, const double* y, const double* heading, const double* kappa, const double* v,
            const double* ax, const double* h, int32_t N, int32_t B, int32_t closed, const rl_stp_query* query,
            int32_t device, rl_stp* out) {
    return one_shot<QueryKind::Stop>({x, y, heading, kappa, v, ax, h, nullptr, nullptr, nullptr, nullptr}, N, B, closed, query, device, out);
}

int rl_retime(const double* x, const double* y, const double* heading, const double* kappa, const double* v,
              const double* ax, const double* h, int32_t N, int32_t B, int32_t closed, const rl_rtm_query* query,
              int32_t device, rl_rtm* out) {
    return one_shot<QueryKind::Retime>({x, y, heading, kappa, v, ax, h, nullptr, nullptr, nullptr, nullptr}, N, B, closed, query, device, out);
}

int rl_recover(const double* x, const double* y, const double* heading, const double* kappa, const double* v,
               const double* ax, const double* h, const double* lo, const double* hi, const double* nx, const double* ny,
               int32_t N, int32_t B, int32_t closed, const rl_rcv_query* query, int32_t device, rl_rcv* out) {
    return one_shot<QueryKind::Recover>({x, y, heading, kappa, v, ax, h, lo, hi, nx, ny}, N, B, closed, query, device, out);
}

int rl_recover_fan(const double* x, const double* y, const double* heading, const double* kappa, const double* v,
                   const double* ax, const double* h, const double* lo, const double* hi, const double* nx, const double* ny,
                   int32_t N, int32_t B, int32_t closed, const rl_fan_query* query, int32_t device, rl_fan* out) {
    return one_shot<QueryKind::Fan>({x, y, heading, kappa, v, ax, h, lo, hi, nx, ny}, N, B, closed, query, device, out);
}

// the rollout stage's kernels (rl_rollout.hip, rl_select.hip's rank) on B host rows and their
// bounds rows: of the rows only x, y, v and the steps go up, no stamps are needed
int rl_rollouts(const double* x, const double* y, const double* heading, const double* kappa, const double* v,
                const double* ax, const double* h, const double* lo, const double* hi, int32_t N, int32_t B,
                int32_t closed, const rl_rll_query* query, int32_t device, rl_rll* out) {
    if (!x || !y || !heading || !kappa || !v || !ax || !h || !lo || !hi || !query || !out)
        return fail(RL_EINVAL, "rl_rollouts: an input row, h, a bounds row, the query or results is NULL");
    if (B < 1 || N < 0) return fail(RL_EINVAL, "rl_rollouts: B < 1 or N < 0");
    if (N > rl::RL_STREAM_MAX_N) return fail(RL_ETOOBIG, "rl_rollouts: N exceeds 1048576");
    int gs = 0;
    if (int rc = check_rollouts(*query, B, &gs)) return rc;
    if (N < 1) return fail(RL_EINVAL, "rollouts: N == 0 (no row)");
    if (int rc = select_device(device)) return rc;
    const size_t BN = (size_t)B * (size_t)N;
    const RllLayout L = rll_layout((size_t)query->Q, (size_t)query->T, (size_t)(query->Q / gs) * (size_t)query->k,
                                   query->v != nullptr, query->row != nullptr, query->seg_hint != nullptr);
    DevArena mem;
    const double* const src[5] = {x, y, v, lo, hi};
    double* d_row[5];
    for (auto& d : d_row) d = mem.get<double>(BN);
    double* d_h = mem.get<double>((size_t)B);
    char* d_qry = mem.get<char>(L.in_bytes);
    char* d_res = mem.get<char>(L.out_bytes);
    if (!mem.ok()) return fail(RL_ENOMEM, "rl_rollouts: hipMalloc failed");
    std::vector<char> block(std::max(L.in_bytes, L.out_bytes));
    rll_pack(*query, L, block.data());
    for (int c = 0; c < 5; ++c)
        if (hipMemcpy(d_row[c], src[c], BN * 8, hipMemcpyHostToDevice) != hipSuccess) return fail(RL_EHIP, "rl_rollouts: upload");
    if (hipMemcpy(d_h, h, (size_t)B * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_qry, block.data(), L.in_bytes, hipMemcpyHostToDevice) != hipSuccess)
        return fail(RL_EHIP, "rl_rollouts: upload");
    rl::TrajParams t{};
    t.x = d_row[0]; t.y = d_row[1]; t.v = d_row[2];
    t.h = d_h;
    t.N = N; t.B = B; t.R = B; t.closed = closed ? 1 : 0;
    if (rll_launch(L, *query, gs, t, d_row[3], d_row[4], d_qry, d_res, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(RL_EHIP, "rl_rollouts: kernel");
    const bool poses = rll_wants_poses(out);
    if (hipMemcpy(block.data(), d_res, poses ? L.out_bytes : L.head_bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(RL_EHIP, "rl_rollouts: download");
    rll_unpack(block.data(), L, out, poses);
    return RL_OK;
}

// rank host scores with rl_rank_kernel (rl_select.hip)
int rl_rank_scores(const double* score, int32_t B, int32_t group_size, int32_t k, int32_t device, int32_t* index) {
    if (!score || !index) return fail(RL_EINVAL, "rl_rank_scores: score / index is NULL");
    int gs = 0;
    if (int rc = check_groups(B, group_size, k, &gs)) return rc;
    if (int rc = select_device(device)) return rc;
    const size_t R = (size_t)(B / gs) * (size_t)k;
    DevArena mem;
    double* d_score = mem.get<double>((size_t)B);
    int32_t* d_index = mem.get<int32_t>(R);
    if (!mem.ok()) return fail(RL_ENOMEM, "rl_rank_scores: hipMalloc failed");
    if (hipMemcpy(d_score, score, (size_t)B * 8, hipMemcpyHostToDevice) != hipSuccess)
        return fail(RL_EHIP, "rl_rank_scores: upload");
    if (rl::launch_rank(d_score, B, gs, k, d_index, nullptr, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(RL_EHIP, "rl_rank_scores: kernel");
    if (hipMemcpy(index, d_index, R * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(RL_EHIP, "rl_rank_scores: download");
    return RL_OK;
}

#ifdef RL_STAMPS
// diagnostic builds only: per-phase cycle totals of the last launch (see rl_kernels.hip)
int rl_debug_stamps(unsigned long long* host, int nblocks) { return rl::debug_stamps(host, nblocks); }
int rl_debug_stamps_stream(unsigned long long* host, int nblocks) { return rl::debug_stamps_stream(host, nblocks); }
int rl_debug_stamps_lat(unsigned long long* host, int nblocks) { return rl::debug_stamps_lat(host, nblocks); }
int rl_debug_stamps_mid(unsigned long long* host, int nblocks) { return rl::debug_stamps_mid(host, nblocks); }
#endif
#ifdef RL_COUNT
// diagnostic builds only: corridor work counters of the stream kernel's translation unit
int rl_debug_counts(unsigned long long* host, int reset) { return rl::debug_counts(host, reset); }
int rl_debug_counts_geom(unsigned long long* host, int reset) { return rl::debug_counts_geom(host, reset); }
int rl_debug_counts_reg(unsigned long long* host, int reset) { return rl::debug_counts_reg(host, reset); }
#endif

}  // extern "C"
