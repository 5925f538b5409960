/*
 * rl_abi.h — C-ABI of the MI355X batched raceline optimizer (steps 7–8 of the
 * reference pipeline).
 *
 * This is the drop-in boundary.  Each entry point replaces one reference
 * function.  "ref" means /root/reference/src/main.cpp (snapshot 2025-10-17).
 *
 *   rl_optimize / rl_plan_*   replace
 *       raceline_min_curv::compute_min_curvature_raceline   (ref:683-764)
 *       raceline_min_time::compute_min_time_raceline         (ref:905-1052)
 *     as called from pipeline::compute_raceline_and_save     (ref:1347-1348)
 *     and pipeline::compute_mintime_and_save                  (ref:1397-1398).
 *   rl_cfg                    mirrors the hot-path subset of cfg::Config (ref:47-119).
 *   rl_cfg_default            mirrors the cfg::Config default initialisers (ref:77-113).
 *   rl_ring_segments          mirrors edges::ringEdges / edges::polylineEdges (ref:251-260).
 *
 * Conventions:
 *   - Plain C types only; the caller owns every buffer; no exception crosses the ABI.
 *   - Return value 0 on success, a negative RL_E* code on failure; rl_last_error()
 *     returns a human-readable message for the calling thread.
 *   - All arithmetic is IEEE fp64.  Points are interleaved [N][2] (x,y), like the
 *     reference's vector<Vec2>.  Segments are [E][4] (x0,y0,x1,y1), like the
 *     reference's vector<pair<Vec2,Vec2>>.
 *   - Results are structure-of-arrays [B][N] (instance-major).
 *   - The compute path is the HIP/gfx950 kernel.  There is no CPU fallback:
 *     with no usable GPU every compute entry point returns RL_ENODEV.
 */
#ifndef RL_ABI_H
#define RL_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RL_ABI_VERSION 6
/* additions that leave every version-6 caller as it is (rl_abi_minor() reports the library's):
 *   1  the lap stage: rl_plan_lap, rl_plan_fetch_lap, rl_plan_select_scored,
 *      rl_optimize_best_scored, rl_path_lengths, rl_plan_kernel_ms indices 4-6 */
#define RL_ABI_MINOR 1

/* error codes */
#define RL_OK          0
#define RL_EINVAL     -1   /* bad argument (NULL pointer, N<0, B<1, n_cfg not 1 or B, ...) */
#define RL_ENODEV     -2   /* no HIP device / device not usable                           */
#define RL_EHIP       -3   /* a HIP runtime call failed                                   */
#define RL_ENOMEM     -4   /* device or host allocation failed                            */
#define RL_ETOOBIG    -5   /* N exceeds what the selected kernel supports                 */

/* optimisation modes (bitmask for rl_plan_create) */
#define RL_MODE_MINCURV 1  /* compute_min_curvature_raceline (ref:683) */
#define RL_MODE_MINTIME 2  /* compute_min_time_raceline      (ref:905) */

/*
 * Hot-path knobs of cfg::Config (ref:47-119).  Field names and meanings are the
 * reference's.  Note the static-initialisation quirk (ref:102): a_total_max is
 * NOT derived from mu at run time; rl_cfg_set_mu() recomputes it the way a
 * recompiled reference would (mu*9.81).
 */
typedef struct rl_cfg {
    double  veh_width_m;         /* ref:77  corridor updates use this (ref:753, 1037)   */
    double  safety_margin_m;     /* ref:78                                               */
    double  lambda_smooth;       /* ref:81                                               */
    int32_t max_outer_iters;     /* ref:82                                               */
    int32_t max_inner_iters;     /* ref:83                                               */
    double  step_init;           /* ref:84                                               */
    double  step_min;            /* ref:85                                               */
    double  armijo_c;            /* ref:86                                               */
    double  kappa_eps;           /* ref:89                                               */
    double  v_cap_mps;           /* ref:90                                               */
    double  mass_kg;             /* ref:93                                               */
    double  Cd;                  /* ref:94                                               */
    double  A_front_m2;          /* ref:95                                               */
    double  rho_air;             /* ref:96                                               */
    double  c_rr;                /* ref:97                                               */
    double  P_max_W;             /* ref:98                                               */
    double  mu;                  /* ref:101 (informational: the hot path reads a_total_max) */
    double  a_total_max;         /* ref:102                                              */
    double  a_lat_max;           /* ref:103                                              */
    double  a_long_acc_cap;      /* ref:104                                              */
    double  a_long_brake_cap;    /* ref:105                                              */
    double  w_time_gain;         /* ref:108                                              */
    double  time_gamma_power;    /* ref:109                                              */
    int32_t time_weight_use_inv_v; /* ref:110 (bool)                                     */
    int32_t max_vpass_iters;     /* ref:112                                              */
    double  inv_v_gain;          /* ref:111                                              */
    int32_t use_total_ge_lat;    /* ref:113 (bool)                                       */
    int32_t _pad0;
} rl_cfg;

/*
 * One track problem: the inputs of compute_*_raceline (ref:683-686, 905-909).
 *   center_xy  [N][2]   centerline samples (closing duplicate already popped, ref:1681-1683)
 *   L                   spline arc length (ref:464); h = L/N (ref:690, 913)
 *   inner_seg  [Ei][4]  inner ring segments (ringEdges / polylineEdges of inner_from_mids)
 *   outer_seg  [Eo][4]  outer ring segments
 *   veh_width           the function argument used for the INITIAL corridor only (ref:706, 930)
 *   closed              closed-loop (periodic) operators when nonzero
 */
typedef struct rl_problem {
    const double* center_xy;
    int32_t       N;
    int32_t       closed;
    double        L;
    const double* inner_seg;
    int32_t       Ei;
    int32_t       Eo;
    const double* outer_seg;
    double        veh_width;
} rl_problem;

/*
 * Caller-allocated results, structure-of-arrays, instance-major [B][N].
 * Any pointer may be NULL to skip that output.  v / ax / lap / vpass_sweeps are
 * written for RL_MODE_MINTIME only.
 *   evals        [B][max_outer_iters]   cost/grad evaluations per outer iteration
 *                                       (the E_k of SURVEY.md §3; 0 for skipped outers)
 *   accepts      [B][max_outer_iters]   accepted PGD steps per outer iteration
 *   vpass_sweeps [B][max_outer_iters+1] v-pass sweeps actually executed per call
 *                                       (early exit once a sweep changes nothing is exact)
 */
typedef struct rl_out {
    double*  x;
    double*  y;
    double*  heading;
    double*  kappa;
    double*  alpha_total;
    double*  alpha_last;
    double*  v;
    double*  ax;
    double*  lap;
    int32_t* evals;
    int32_t* accepts;
    int32_t* vpass_sweeps;
} rl_out;

/* ---------------------------------------------------------------- config */
void rl_cfg_default(rl_cfg* cfg);
/* mu sweep helper: sets mu and a_total_max = mu*9.81 (ref:101-102) */
void rl_cfg_set_mu(rl_cfg* cfg, double mu);

/* ------------------------------------------------------------- geometry
 * Ring → segments, like edges::ringEdges (closed, ref:251-255: n segments with wrap)
 * or edges::polylineEdges (open, ref:256-260: n-1 segments).  seg_out must hold
 * [n][4] doubles.  Returns the number of segments written (>=0) or RL_EINVAL.     */
int rl_ring_segments(const double* ring_xy, int32_t n, int32_t closed, double* seg_out);

/* α-seed of instance b at sample i (build-defined):
 *   seed 0            -> 0.0 (the reference starts from α≡0, ref:720)
 *   otherwise         -> sigma * xi, xi ~ U(-1,1) from splitmix64(seed, i),
 * clamped to the initial corridor [lo_i, hi_i] by the optimizer itself.          */
double rl_seed_value(uint64_t seed, int32_t i, double sigma);
#define RL_SEED_SIGMA 0.25

/* ------------------------------------------------------------ one-shot
 * Optimise B instances of one problem.  cfg has n_cfg entries (1 = broadcast,
 * or B = one per instance).  seeds has B entries or is NULL (all zero = exactly
 * the reference).  out_mincurv / out_mintime may be NULL to skip that mode.
 * Synchronous: host buffers in, host buffers out (PCIe included), on the calling
 * thread's current HIP device.  Device plans and pinned staging buffers are reused
 * across calls from a small process-wide cache keyed by (device, N, B, n_cfg,
 * max_outer_iters, closed, kernel variant) and the ring segments (bitwise): a repeat
 * call uploads only the centreline, cfg and seeds.  rl_lap_eval shares the cache.  */
int rl_optimize(const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg,
                const uint64_t* seeds, int32_t B,
                rl_out* out_mincurv, rl_out* out_mintime);
/* Timing of this thread's last successful rl_optimize / rl_lap_eval: *kernel_ms = HIP-event
 * time from the first to the last kernel of the call, *call_ms = wall time of the whole
 * call (uploads, kernels, downloads into the caller's buffers).  Either may be NULL.    */
int rl_last_call_ms(float* kernel_ms, float* call_ms);
/* The same call's times split: *run_ms = the run bracket (as rl_last_call_ms' kernel_ms:
 * first kernel start to last kernel end), *mincurv_ms / *mintime_ms = each optimiser kernel
 * alone from its own start and end events (-1 when that mode did not run), *call_ms = wall
 * time of the whole call.  Any pointer may be NULL. */
int rl_last_call_times(float* run_ms, float* mincurv_ms, float* mintime_ms, float* call_ms);
/* How the same call downloaded its results.  Calls whose results exceed 8 MiB overlap the
 * download with the kernel: every instance signals its completion into pinned host memory,
 * and each group of completed instances (16 per optimiser) is copied out while later
 * instances still compute (RL_OVERLAP_DOWNLOAD=0 in the environment turns this off).
 * *groups = the groups of the call (0: one download after the kernel), *groups_signalled =
 * those queued on their instances' flags (the rest waited for the kernel's end).  Either
 * pointer may be NULL.  (Not in the reference: the drop-in's own transfer path.) */
int rl_last_call_download(int32_t* groups, int32_t* groups_signalled);
/* Free the idle plans and pinned buffers of the cache (device memory returns to HIP). */
int rl_release_plan_cache(void);
/* Idle plans in the cache and the device / pinned host bytes they hold.  The cache keeps
 * at most 8 idle plans and RL_PLAN_CACHE_MB (environment, default 2048) MiB of device plus
 * pinned memory, evicting the least recently used; a plan larger than that on its own is
 * released when its call returns.  Any pointer may be NULL. */
int rl_plan_cache_info(int32_t* entries, int64_t* device_bytes, int64_t* pinned_bytes);

/* ------------------------------------------------------------ multi-device
 * rl_optimize over n_dev devices (SURVEY.md §8b device list, §8e): the B instances are
 * split into contiguous blocks (block d = instances [B*d/n, B*(d+1)/n), n = min(n_dev, B)),
 * one plan and HIP stream per device, all devices enqueued before the first download;
 * each block's results are copied to its offset of the caller's host outputs (the final
 * gather).  devices: n_dev device indices (a device may repeat: two plans on one device),
 * or NULL for 0..n_dev-1.  Same cfg/seeds/out conventions as rl_optimize; every cfg is
 * checked before any device work.  Every block runs the kernel shape rl_optimize picks for
 * the whole batch B (rl_plan_set_shape_batch), so on devices with the same CU count the
 * results equal rl_optimize's bit for bit, counters included (the shapes sum J and the
 * lap in different tree orders).  The calling thread's current device is unchanged on
 * return. */
int rl_optimize_multi(const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg,
                      const uint64_t* seeds, int32_t B, const int32_t* devices, int32_t n_dev,
                      rl_out* out_mincurv, rl_out* out_mintime);

/* ---------------------------------------------------- device-resident plan
 * For repeated runs with inputs already resident in HBM (bench, services).
 * create: allocates device buffers on `device` and uploads the inputs.
 * run:    enqueues the optimisation on `hip_stream` (a hipStream_t; NULL = the
 *         plan's own stream) and returns immediately.  With both modes and a batch
 *         that leaves the GPU partly idle (B x waves per instance <= 8 x CUs), the
 *         min-time kernel runs on a second plan-owned stream, concurrently with the
 *         min-curvature kernel; `hip_stream` waits for both.
 * fetch:  copies results to host (synchronises the stream used by run).
 * device_outputs: device pointers of the result arrays (for collectives).       */
typedef struct rl_plan rl_plan;

int rl_plan_create(rl_plan** plan, int32_t device, const rl_problem* prob,
                   const rl_cfg* cfg, int32_t n_cfg, const uint64_t* seeds,
                   int32_t B, int32_t modes);
int rl_plan_run(rl_plan* plan, void* hip_stream);
/* rl_plan_run of n plans of one device in as few launches as their kernel shapes allow (a
 * sweep of many small plans: C4's 14 (track, mode) plans of 512 one-wave instances).  Every
 * (plan, mode) whose shape is a one-wave throughput shape ((4|5|8, 64): N <= 512 in a batch
 * that fills the GPU) joins one launch with the other plans of its mode, K and closed flag
 * (up to 8 plans per launch), the instances of all of them in one grid; other
 * plans run as rl_plan_run.  The launches run concurrently on plan-owned streams, after
 * everything queued on `hip_stream` (NULL: the first plan's stream), which waits for all of
 * them.  Results equal each plan's own rl_plan_run bit for bit.  A plan may appear once. */
int rl_plan_run_group(rl_plan* const* plans, int32_t n, void* hip_stream);
int rl_plan_fetch(rl_plan* plan, rl_out* out_mincurv, rl_out* out_mintime);
/* which: RL_MODE_MINCURV or RL_MODE_MINTIME; fills device pointers (same layout as
 * rl_out, NULL where the mode does not produce the field). */
int rl_plan_device_outputs(rl_plan* plan, int32_t which, rl_out* dev_out);
/* Bind caller-owned DEVICE buffers (same layout as rl_out: [B][N] arrays, lap [B],
 * evals/accepts [B][max_outer_iters], vpass_sweeps [B][max_outer_iters+1]) as the
 * result storage of mode `which`; NULL fields keep the plan's own buffers.  Lets a
 * framework (e.g. torch tensors for an RCCL gather) receive results without copies. */
int rl_plan_bind_device_outputs(rl_plan* plan, int32_t which, const rl_out* dev_out);
/* device time of the last run, in ms, measured with HIP events on the run stream:
 * idx 0 = the whole run, 1 = the min-curvature kernel, 2 = the min-time kernel, 3 = the
 * selection stage of the last rl_plan_select (score, rank and gather kernels), 4 = the lap
 * stage of the last rl_plan_lap (5 = its preparation kernel, 6 = its evaluation kernel), 7 =
 * the trajectory stage of the last rl_plan_trajectory, 8 = the horizon stage of the last
 * rl_plan_horizon, 9 = the rejoin stage of the last rl_plan_rejoin, 10 = the stop stage of the
 * last rl_plan_stop, 11 = the bounds stage of the last rl_plan_bounds, 12 = the bounds at the
 * horizon stage's ticks of the last rl_plan_horizon_bounds, 13 = the retime stage of the last
 * rl_plan_retime, 14 = the recover stage of the last rl_plan_recover, 15 = the fan stage of the
 * last rl_plan_recover_fan, 16 = the rollout stage of the last rl_plan_rollouts (its locate and
 * rank kernels together). */
int rl_plan_kernel_ms(rl_plan* plan, int32_t idx, float* ms);
/* The batch size the plan's kernel shape is chosen for (rl_kernel_shape's B); 0 = the plan's
 * own B (the default).  Shapes differ in the tree order of the J / decrease / lap sums, so
 * the last bits of J and the lap (and on a near-tie an Armijo decision) can depend on the
 * shape: plans that must give identical results take the same shape batch.  Plans that run
 * concurrently on one device should pass the total instance count in flight, so that none
 * takes a latency shape meant to spread its instances over the whole GPU.  Takes effect
 * at the next rl_plan_run. */
int rl_plan_set_shape_batch(rl_plan* plan, int32_t shape_B);
/* The kernel shape rl_plan_run launches for `mode` (K = 0: the streaming kernel). */
int rl_plan_shape(rl_plan* plan, int32_t mode, int32_t* K, int32_t* T);
int rl_plan_destroy(rl_plan* plan);

/* ------------------------------------------------- selection: the best k of a batch
 * The stage after the optimiser (not in the reference: a multi-start caller's last step).
 * The B instances of a plan form G = B / group_size contiguous groups; every instance gets
 * a score, the k best of each group are ranked on the device, and only their rows are
 * copied into compact buffers and downloaded (G*k rows instead of B).
 *   score, RL_MODE_MINTIME:  the lap time lap[b] the optimiser wrote.
 *   score, RL_MODE_MINCURV:  h * sum_i kappa[b][i]^2 with h = L/N (L[b]/N for plans with
 *                            per-instance lengths), summed in an order fixed by N alone, so
 *                            its bits do not depend on B, the grouping, k or the kernel shape.
 *   order: ascending in (isnan(score), score, instance index): scores compare as IEEE
 *          values (-inf first, +inf before any NaN, -0.0 and +0.0 tie), NaNs rank last,
 *          equal scores (and NaNs among themselves) rank by the lower index.
 * Min-curvature racelines can also be ranked by their lap time (the reference's debug-dump
 * "min-curv lap"): the lap stage below and RL_SCORE_LAP.  rl_optimize_multi and the device
 * list are not extended: the selection runs on one device. */
#define RL_SELECT_MAX_K 64
typedef struct rl_select {
    int32_t mode;        /* RL_MODE_MINCURV or RL_MODE_MINTIME (exactly one): whose results are ranked */
    int32_t k;           /* winners per group, 1..min(group_size, RL_SELECT_MAX_K)                      */
    int32_t group_size;  /* instances per group; 0 = B (one group); B % group_size == 0                 */
    int32_t _pad;
} rl_select;

/* Enqueue score -> rank -> gather after the plan's last run, on the stream that run used
 * (hip_stream NULL; another stream is first made to wait for the run).  Reads the result
 * arrays in force (after rl_plan_bind_device_outputs: the caller's).  The selection buffers
 * are plan-owned, allocated at the first call and when G*k grows.  RL_EINVAL before any
 * device work for: a NULL argument, a mode that is not exactly one of the plan's, k < 1,
 * k > group_size, k > RL_SELECT_MAX_K, B % group_size != 0, N == 0, a plan never run. */
int rl_plan_select(rl_plan* plan, const rl_select* sel, void* hip_stream);
/* Download the last selection (synchronises its stream): index, score [G][k] (index holds
 * global instance indices, best first; score = the winners' scores); all_scores [B] or NULL;
 * out: rl_out whose arrays hold G*k rows, row g*k + r = instance index[g][r] (NULL, or NULL
 * fields, are skipped).  RL_EINVAL before a select, or after a run that followed it. */
int rl_plan_fetch_selected(rl_plan* plan, int32_t* index, double* score, double* all_scores, rl_out* out);
/* rl_optimize for `sel->mode` only, without the full download: upload, kernel, select,
 * download of the G*k rows.  Plans come from rl_optimize's cache; rl_last_call_times reports
 * the call (rl_last_call_download: 0 groups). */
int rl_optimize_best(const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg, const uint64_t* seeds, int32_t B,
                     const rl_select* sel, int32_t* index, double* score, double* all_scores, rl_out* out);
/* Rank caller-supplied scores [B] (host in, host out) with the same kernel: index [G][k]. */
int rl_rank_scores(const double* score, int32_t B, int32_t group_size, int32_t k, int32_t device, int32_t* index);

/* ------------------------------------------------- lap stage: min-curvature racelines by lap time
 * The debug dump's "min-curv lap" (ref:1443-1450, 1472-1479) for every instance of a plan, on
 * the device: the min-curvature raceline's own path length
 *   L_mc[b] = (((0.0 + d_0) + d_1) + ...),  d_i = hypot(x[i+1]-x[i], y[i+1]-y[i]),
 * in index order with the closing segment last (closed tracks; N <= 1: 0.0), bit for bit
 * the reference's path_length; then heading, curvature and velocity_profile_forward_backward
 * with h = L_mc[b]/N, by the min-time kernel at max_outer_iters = 0, exactly as rl_lap_eval
 * runs it on the same B paths and lengths (the same kernel shape, so the same bits). */
#define RL_SCORE_DEFAULT 0   /* lap for min-time, h*sum kappa^2 for min-curvature (rl_plan_select) */
#define RL_SCORE_LAP     1   /* the lap stage's lap; differs from DEFAULT only for RL_MODE_MINCURV */

/* Enqueue the lap stage after the plan's last run (stream rules of rl_plan_select).  Reads the
 * min-curvature x, y arrays in force (after rl_plan_bind_device_outputs: the caller's); its
 * buffers are plan-owned, allocated at the first call.  A later run invalidates the stage.
 * RL_EINVAL before any device work for: a NULL plan, a plan without RL_MODE_MINCURV, a plan
 * never run, N == 0. */
int rl_plan_lap(rl_plan* plan, void* hip_stream);
/* Download the lap stage (synchronises its stream): out receives heading, kappa (both with
 * h = L_mc/N), v, ax [B][N], lap [B] and vpass_sweeps [B][1]; its other fields are skipped.
 * path_len [B] (or NULL) receives L_mc.  RL_EINVAL before a lap stage, or after a run that
 * followed it. */
int rl_plan_fetch_lap(rl_plan* plan, rl_out* out, double* path_len);
/* rl_plan_select with a choice of score.  RL_SCORE_DEFAULT, or any score with
 * RL_MODE_MINTIME: exactly rl_plan_select.  RL_SCORE_LAP with RL_MODE_MINCURV: runs the lap
 * stage unless one is valid since the last run, ranks its lap, and gathers the winners: x, y,
 * heading, kappa, alpha_total, alpha_last, evals, accepts are the optimiser's rows (as the
 * full download), v, ax, lap and vpass_sweeps [G*k][1] the lap stage's; rl_plan_fetch_selected
 * then fills those four too.  An unknown score is RL_EINVAL. */
int rl_plan_select_scored(rl_plan* plan, const rl_select* sel, int32_t score, void* hip_stream);
/* rl_optimize_best with that score (rl_optimize_best is RL_SCORE_DEFAULT). */
int rl_optimize_best_scored(const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg, const uint64_t* seeds, int32_t B,
                            const rl_select* sel, int32_t score, int32_t* index, double* score_out,
                            double* all_scores, rl_out* out);
/* The path lengths L[b] of B paths given as rows x[B][N], y[B][N] (host in, host out), summed
 * as above by the lap stage's preparation kernel.  RL_EINVAL for a NULL argument, B < 1 or
 * N < 0; RL_ETOOBIG for N > 1048576. */
int rl_path_lengths(const double* x, const double* y, int32_t N, int32_t B, int32_t closed,
                    int32_t device, double* L_out);

/* ------------------------------------------------- trajectory stage: racelines by time
 * What a controller tracks is the state at every control tick, not at every h metres.  The
 * stage after the optimiser, the lap stage and the selection, on the device: for one row
 * (x, y, heading, kappa, v, ax of N samples, step h, closed or open), in fp64 without
 * contraction,
 *   stamps  t_0 = 0,  t_{i+1} = t_i + h / max(1e-6, v_i)  for i = 0 .. N-1, added serially in
 *           index order (the reference's lap loop, ref:854-860); S = closed ? N : N-1 segments,
 *           segment i from sample i to sample j = (i+1) mod N;  T = t_S  (N == 0, and an open
 *           row of one sample: T = 0)
 *   ticks   tau_m = (double)m * dt,  M = min(M_cap, #{m : tau_m < T})  (strict);  T NaN or
 *           infinite: M = 0
 *   segment of a tick: the i in [0, S) with t_i <= tau_m < t_{i+1};  u = (tau_m - t_i) / (t_{i+1} - t_i)
 *   s = ((double)i + u) * h;  x = x_i + u*(x_j - x_i), and y, v, kappa likewise;
 *   heading = psi_i + u*d, d = psi_j - psi_i, less 2*pi if d > pi, plus 2*pi if d < -pi;
 *   ax = ax_i (constant on a segment, ref:858).
 * raceline.trajectory_host states the same in NumPy; the kernel equals it bit for bit.
 * For closed rows T is the reference's lap summed serially; the optimiser's own `lap` sums the
 * same terms as a tree and may differ from T in the last bits (by at most (N+2)*2^-52
 * relative).  The stamp order is the contract, as the order of L_mc is for the lap stage.
 * This is an addition to ABI 6.1 that leaves RL_ABI_MINOR as it is: callers discover it
 * through rl_abi_features(). */
typedef struct rl_traj {      /* caller-allocated; [R][M_cap] unless noted; NULL fields skipped */
    double *s, *x, *y, *heading, *kappa, *v, *ax;
    double *stamps;           /* [R][N+1] */
    double *T;                /* [R] */
    int32_t *count;           /* [R]  = M; ticks m >= count[r] of row r are unspecified */
} rl_traj;
#define RL_TRAJ_ALL 0         /* R = B: output row r is instance r */
#define RL_TRAJ_SELECTED 1    /* R = G*k: output row g*k + r is instance index[g][r] of the plan's valid selection */
#define RL_TRAJ_MAX_TICKS 1048576

/* Enqueue the stage after the plan's last run (stream rules of rl_plan_select; a later run
 * invalidates it).  mode RL_MODE_MINTIME reads the min-time rows in force (after
 * rl_plan_bind_device_outputs: the caller's) with h = L/N (L[b]/N for per-instance lengths).
 * mode RL_MODE_MINCURV reads the optimiser's x, y and the lap stage's heading, kappa, v, ax
 * with h = L_mc[b]/N, and runs rl_plan_lap first unless a lap stage is valid since the last
 * run.  rows RL_TRAJ_SELECTED resamples only the winners of the plan's valid selection, which
 * must be of the same mode.  The buffers are plan-owned (they count toward the plan cache's
 * budget), allocated at the first call and when R or M_cap grows.  rl_plan_kernel_ms index 7
 * is the stage.  RL_EINVAL before any device work for: a NULL plan, a mode that is not exactly
 * one of the plan's, dt not finite or <= 0, M_cap < 1 or > RL_TRAJ_MAX_TICKS, N == 0, an unknown
 * `rows`, a plan never run, RL_TRAJ_SELECTED without a valid selection of `mode`. */
int rl_plan_trajectory(rl_plan* plan, int32_t mode, int32_t rows, double dt, int32_t M_cap, void* hip_stream);
/* Download the last trajectory stage (synchronises its stream) into the non-NULL fields of
 * out.  RL_EINVAL before a stage, or after a run that followed it. */
int rl_plan_fetch_trajectory(rl_plan* plan, rl_traj* out);
/* rl_optimize_best_scored, then the trajectories of the winners (RL_TRAJ_SELECTED), with the
 * winners' rows and trajectories downloaded in one pass: traj holds G*k rows. */
int rl_optimize_best_trajectory(const rl_problem* prob, const rl_cfg* cfg, int32_t n_cfg, const uint64_t* seeds, int32_t B,
                                const rl_select* sel, int32_t score, int32_t* index, double* score_out,
                                double* all_scores, rl_out* out, double dt, int32_t M_cap, rl_traj* traj);
/* The trajectories of B given rows [B][N] with steps h [B] (host in, host out; R = B) by the
 * same kernel.  N == 0 gives T = 0 and count = 0.  RL_EINVAL for a NULL input or out, B < 1,
 * N < 0, a bad dt or M_cap; RL_ETOOBIG for N > 1048576. */
int rl_trajectory(const double* x, const double* y, const double* heading, const double* kappa,
                  const double* v, const double* ax, const double* h, int32_t N, int32_t B,
                  int32_t closed, double dt, int32_t M_cap, int32_t device, rl_traj* out);

/* ------------------------------------------------- horizon stage: look-ahead from a pose
 * A controller asks every 10-50 ms: "I am at (px, py); where on the raceline is that, and what
 * are the next M ticks from there?"  The stage after a trajectory stage, as often as the
 * caller likes without another run: each of Q query poses is located on one row of that stage
 * (an exact nearest point on the polyline, optionally within a window of segments around a
 * hint) and up to M_cap ticks are resampled from the located time on, dt apart; on a closed
 * row they run on across the start line.  Only the poses go up; only the ticks and the
 * location come down.  In fp64 without contraction, with smax(a,b) = (a<b)?b:a and
 * smin(a,b) = (b<a)?b:a; one row is the trajectory stage's: samples x, y, psi, kappa, v, ax [N],
 * step h, stamps t[0..N], T = t_S, S = closed ? N : N-1 segments, segment i from sample i to
 * j = (i+1) mod N:
 *   candidates  seg_hint = -1: every i in [0, S).  Hint g, window W >= 0, closed row:
 *           (g + k) mod S for k = -W .. W, and all of [0, S) if 2W+1 >= S.  Open row:
 *           max(0, g-W) .. min(S-1, g+W).
 *   distance of pose p to candidate i:  dx = x_j - x_i, dy = y_j - y_i, wx = px - x_i,
 *           wy = py - y_i, dd = dx*dx + dy*dy, c = wx*dx + wy*dy,
 *           u = dd > 0 ? smin(1.0, smax(0.0, c/dd)) : 0.0, rx = wx - u*dx, ry = wy - u*dy,
 *           D = rx*rx + ry*ry
 *   winner  the candidate least in the order (isnan(D), D, i): the lowest segment index wins a
 *           tie.  A NaN winner, or S = 0: seg = -1 and count = 0, nothing else is specified.
 *   location  seg = i, u, dist2 = D;  e = (dx*wy - dy*wx) < 0 ? -sqrt(D) : sqrt(D), the lateral
 *           offset, left of the direction of travel positive;  t0 = t_i + u*(t_{i+1} - t_i);
 *           s0 = ((double)i + u)*h
 *   ticks   tau_m = t0 + (double)m*dt.  Open rows: count = min(M_cap, #{m : tau_m < T}), wrap
 *           count c = 0, w = tau_m.  Closed rows: count = M_cap if T is finite and > 0, else 0;
 *           c = floor(tau_m / T), w = tau_m - c*T (two roundings), then at most one fix-up each
 *           way: w < 0: w += T, c -= 1; else w >= T: w -= T, c += 1 (c stays a double).
 *   segment of a tick: i = clip(#{k <= S : t_k <= w} - 1, 0, S-1), the trajectory stage's
 *           bisection on w;  u_m = (w - t_i)/(t_{i+1} - t_i)
 *   columns s = ((c*(double)S + (double)i) + u_m)*h (monotone across laps; for c = 0 the bits
 *           of the trajectory stage's s); x, y, heading (shorter arc), kappa, v, ax: the
 *           trajectory stage's expressions with u_m.
 * raceline.horizon_host states the same in NumPy; the kernel equals it bit for bit.  These are
 * additions to ABI 6.1 that leave RL_ABI_MINOR as it is: RL_FEATURE_HORIZON announces them. */
typedef struct rl_hzn_query {
    const double*  pose_xy;   /* [Q][2] host */
    const int32_t* row;       /* [Q] row of the plan's trajectory stage (of B for rl_horizon); NULL: 0 */
    const int32_t* seg_hint;  /* [Q], -1 = every segment; NULL: all -1 */
    int32_t Q, window, M_cap, _pad;
    double  dt;
} rl_hzn_query;

typedef struct rl_hzn {       /* caller-allocated; NULL fields skipped */
    double *s, *x, *y, *heading, *kappa, *v, *ax;   /* [Q][M_cap]; ticks m >= count[q] are unspecified */
    double *u, *t0, *s0, *e, *dist2;                /* [Q] */
    int32_t *seg, *count;                           /* [Q] */
} rl_hzn;

#define RL_HZN_MAX_QUERIES 65536

/* Enqueue the stage after the plan's last trajectory stage, whose rows, stamps and T it reads
 * (stream rules of rl_plan_select).  It may be repeated with other poses without a run or a
 * trajectory stage in between, and leaves the trajectory stage as it is; a later rl_plan_run or
 * rl_plan_trajectory invalidates it.  The buffers are plan-owned (they count toward the plan
 * cache's budget) and grow with Q and M_cap.  pose_xy, row and seg_hint are read before the
 * call returns.  rl_plan_kernel_ms index 8 is the stage.  RL_EINVAL before any device work for:
 * a NULL plan, query or pose_xy, Q < 1 or > RL_HZN_MAX_QUERIES, window < 0, dt not finite or
 * <= 0, M_cap < 1 or > RL_TRAJ_MAX_TICKS, a row outside the stage's [0, R), a hint outside
 * [-1, S), a plan with no valid trajectory stage, and a trajectory stage whose source rows have
 * been replaced since (a selection after a stage of RL_TRAJ_SELECTED, a lap stage after a
 * stage of RL_MODE_MINCURV). */
int rl_plan_horizon(rl_plan* plan, const rl_hzn_query* query, void* hip_stream);
/* Download the last horizon stage (synchronises its stream) into the non-NULL fields of out.
 * RL_EINVAL before a stage, or after a run or trajectory stage that followed it. */
int rl_plan_fetch_horizon(rl_plan* plan, rl_hzn* out);
/* The horizons of poses on B given rows [B][N] with steps h [B] (host in, host out): the
 * trajectory kernel for the stamps, then the horizon kernel.  RL_EINVAL for a NULL input, query
 * or out, B < 1, N < 1 and the query errors above with R = B; RL_ETOOBIG for N > 1048576. */
int rl_horizon(const double* x, const double* y, const double* heading, const double* kappa,
               const double* v, const double* ax, const double* h, int32_t N, int32_t B,
               int32_t closed, const rl_hzn_query* query, int32_t device, rl_hzn* out);

/* ------------------------------------------------- rejoin stage: a reachable profile from the car's speed
 * The horizon stage's ticks carry the row's own v and ax, the flying-lap profile.  A car that is
 * not on that profile (a standing start, a slow corner exit, a late brake) cannot follow them.
 * This stage takes the car's speed v0 and one rl_cfg, the car's limits now (they may differ from
 * the planning cfg), marches the reachable speed nearest the row's from the located point until
 * it meets the row's, and resamples the ticks along that profile; after the merge they are the
 * row's own.  In fp64 without contraction, smax / smin and the row as for the horizon stage:
 *   ax_max_at(cfg, w, k) -> (a_acc, a_brk), the reference's lambda (ref:797-824):
 *           alat = w*w*fabs(k);  a_total = use_total_ge_lat ? smax(a_total_max, a_lat_max) : a_total_max;
 *           a_res = sqrt(smax(0.0, a_total*a_total - alat*alat));
 *           Fd = 0.5*rho_air*Cd*A_front_m2*w*w;  Fr = mass_kg*9.81*c_rr;
 *           a_power = (P_max_W > 0 && w > 1e-6) ? (P_max_W/(mass_kg*w) - (Fd + Fr)/mass_kg) : 1e9;
 *           a_acc = smax(0.0, smin(smin(a_res, a_long_acc_cap), a_power));
 *           a_brk = smax(0.0, smin(a_res, a_long_brake_cap) + (Fd + Fr)/mass_kg)
 *           (a_total*a_total, 0.5*rho_air*Cd*A_front_m2 and mass_kg*9.81*c_rr are evaluated once,
 *           left to right)
 *   locate  the horizon stage's candidates, distance, winner and location, with the same seg_hint
 *           and window: seg = i, u, e, dist2, t0, s0.  A NaN winner, or S = 0: seg = -1,
 *           count = 0, merge_node = -1, nothing else is specified.
 *   nodes   node 0 is the located point: kappa_0 = kappa_i + u*(kappa_j - kappa_i),
 *           r_0 = v_i + u*(v_j - v_i), d_0 = (1.0 - u)*h.  Node k >= 1 is sample n_k = i + k
 *           (unwrapped; row index n_k mod N on a closed row): kappa_k, r_k that sample's kappa
 *           and v, d_k = h.  K_lim = min(K_cap, closed ? N : N-1-i).
 *   march   serial, in index order: w_0 = v0, tt_0 = 0.0.  If w_0 == r_0: K* = 0.  Otherwise for
 *           k = 0, 1, ...:  (a_acc, a_brk) = ax_max_at(cfg, w_k, kappa_k);
 *           up = sqrt(smax(0.0, w_k*w_k + (2.0*a_acc)*d_k));
 *           dn = sqrt(smax(0.0, w_k*w_k - (2.0*a_brk)*d_k));
 *           w_{k+1} = smin(up, smax(dn, r_{k+1}))   (the reachable speed nearest the row's);
 *           tt_{k+1} = tt_k + (2.0*d_k)/smax(1e-6, w_k + w_{k+1})   (exact for constant
 *           acceleration, finite from standstill).  The first k+1 with w_{k+1} == r_{k+1} is the
 *           merge node K*; none by K_lim: K* = -1.  K_end = K* >= 0 ? K* : K_lim.
 *           overspeed = #{k in [0, K_end] : w_k > r_k}.
 *   merge   c0 = floor(n_K* / N), j* = n_K* - c0*N, t_ref = (K* == 0) ? t0 : t[j*];
 *           t_merge = tt_{K_end} (the time marched);
 *           t_loss = tt_K* - (((double)c0*T + t_ref) - t0), the time lost against the row's own
 *           schedule (a quiet NaN when K* = -1).  From standstill at sample 0, T + t_loss is the
 *           standing-start lap.
 *   ticks   tau_m = (double)m*dt, counted from the car.  M1 = #{m < M_cap : tau_m < tt_{K_end}}
 *           ticks lie on the march: k = the node with tt_k <= tau_m < tt_{k+1} (bisection:
 *           a = 0, e = K_end; while e - a > 1: mid = a + (e-a)/2; tt_mid <= tau_m ? a = mid : e = mid),
 *           u_m = (tau_m - tt_k)/(tt_{k+1} - tt_k); x, y, heading (shorter arc) and kappa are
 *           interpolated with u_m between the node values (node 0's: the trajectory stage's
 *           expressions with u; its kappa is kappa_0); v = w_k + u_m*(w_{k+1} - w_k);
 *           ax = d_k > 0 ? (w_{k+1}*w_{k+1} - w_k*w_k)/(2.0*d_k) : 0.0;
 *           s = s_k + u_m*(s_{k+1} - s_k), s_0 = s0, s_k = (double)n_k*h.
 *           Not merged: count = M1.  Merged: tick m >= M1 has the row time
 *           w_ref = t_ref + (tau_m - tt_K*); the horizon stage's wrap (c, w of w_ref), bisection
 *           and columns follow, with the lap count c0 + c in its s.  Open rows:
 *           count = M1 + #{M1 <= m < M_cap : w_ref < T}; closed rows: count = M_cap if T is
 *           finite and > 0, else M1.
 * A pose with v0 == r_0 therefore reproduces the horizon stage bit for bit.
 * raceline.rejoin_host states the same in NumPy; the kernel equals it bit for bit.  These are
 * additions to ABI 6.1 that leave RL_ABI_MINOR as it is: RL_FEATURE_REJOIN announces them. */
#define RL_RJN_MAX_NODES 1024
typedef struct rl_rjn_query {
    const double*  pose_xy;   /* [Q][2] host */
    const int32_t* row;       /* [Q] row of the plan's trajectory stage (of B for rl_rejoin); NULL: 0 */
    const int32_t* seg_hint;  /* [Q], -1 = every segment; NULL: all -1 */
    int32_t Q, window, M_cap, _pad;
    double  dt;
    const double*  v0;        /* [Q] the car's speed, finite and >= 0 */
    const rl_cfg*  cfg;       /* one: the car's limits now */
    int32_t K_cap, _pad2;     /* march nodes, 1..RL_RJN_MAX_NODES */
} rl_rjn_query;

typedef struct rl_rjn {       /* caller-allocated; NULL fields skipped */
    double *s, *x, *y, *heading, *kappa, *v, *ax;   /* [Q][M_cap]; ticks m >= count[q] are unspecified */
    double *u, *t0, *s0, *e, *dist2;                /* [Q] */
    int32_t *seg, *count;                           /* [Q] */
    int32_t *merge_node, *overspeed;                /* [Q] */
    double *t_merge, *t_loss;                       /* [Q] */
    double *node_v, *node_t;                        /* [Q][K_cap+1] w_k, tt_k; entries past K_end are unspecified;
                                                       downloaded only when asked for */
} rl_rjn;

/* Enqueue the stage after the plan's last trajectory stage: rl_plan_horizon's stream, validity
 * and invalidation rules.  It leaves the trajectory stage, the last horizon stage and the
 * results untouched; its buffers are plan-owned (they count toward the plan cache's budget) and
 * grow with Q, M_cap and K_cap.  The query's arrays and cfg are read before the call returns.
 * rl_plan_kernel_ms index 9 is the stage.  RL_EINVAL before any device work for: every error
 * of rl_plan_horizon, a NULL cfg or v0, a v0[q] that is not finite or is < 0, K_cap < 1 or
 * > RL_RJN_MAX_NODES. */
int rl_plan_rejoin(rl_plan* plan, const rl_rjn_query* query, void* hip_stream);
/* Download the last rejoin stage (synchronises its stream) into the non-NULL fields of out.
 * RL_EINVAL before a stage, or after a run or trajectory stage that followed it. */
int rl_plan_fetch_rejoin(rl_plan* plan, rl_rjn* out);
/* The same on B given rows [B][N] with steps h [B] (host in, host out): the trajectory kernel
 * for the stamps, then the rejoin kernel.  Errors as rl_horizon's, and the query errors above. */
int rl_rejoin(const double* x, const double* y, const double* heading, const double* kappa,
              const double* v, const double* ax, const double* h, int32_t N, int32_t B,
              int32_t closed, const rl_rjn_query* query, int32_t device, rl_rjn* out);

/* ------------------------------------------------- stop stage: brake to a target speed at a sample
 * The horizon and rejoin stages serve profiles that are periodic or open-ended.  This stage
 * answers "be at speed v_target when you reach sample J": the stop after the finish line, the
 * stop before the end of the visible track, the slow zone.  It is the rejoin stage's query with
 * a target.  A brake envelope is swept backward from the target with the car's cfg, the car's
 * speed is marched forward under it, and the ticks follow the march up to the target.  Inside
 * the envelope the envelope caps the speed, so a car that starts inside it meets the target.
 * In fp64 without contraction; smax, smin, the row and ax_max_at are the rejoin stage's:
 *   locate, nodes   the rejoin stage's: seg = i, u, e, dist2, t0, s0; kappa_k, r_k, d_k,
 *           n_k = i + k for k = 0..K_lim, K_lim = min(K_cap, closed ? N : N-1-i).  A NaN winner,
 *           or S = 0: seg = -1, stop_node = -1, count = 0, nothing else is specified.
 *   target  J = stop_sample[q].  Closed rows: K_s = ((J - i - 1) mod N + N) mod N + 1, in
 *           [1, N], the first time sample J comes up ahead of the located segment (J == i:
 *           K_s = N, J == i + 1: K_s = 1).  Open rows: K_s = J - i.  K_s < 1 or K_s > K_lim:
 *           out of range, stop_node = -1, count = 0, the location (seg, u, t0, s0, e, dist2) is
 *           still written and nothing else is specified; the caller falls back on the rejoin
 *           or the horizon stage.
 *   envelope   serial, backward: b_{K_s} = v_target.  For k = K_s-1 .. 0:
 *           (., a_brk) = ax_max_at(cfg, b_{k+1}, kappa_{k+1});
 *           b_k = sqrt(smax(0.0, b_{k+1}*b_{k+1} + (2.0*a_brk)*d_k))
 *           (the reference's backward sweep with the car's cfg).  reachable = (v0 <= b_0).
 *   march   serial, forward, always to K_s (no early exit, no special case for v0 == r_0):
 *           w_0 = v0, tt_0 = 0.0.  For k = 0 .. K_s-1:
 *           (a_acc, a_brk) = ax_max_at(cfg, w_k, kappa_k);
 *           up = sqrt(smax(0.0, w_k*w_k + (2.0*a_acc)*d_k));
 *           dn = sqrt(smax(0.0, w_k*w_k - (2.0*a_brk)*d_k));
 *           w_{k+1} = smin(up, (w_k <= b_k) ? smin(b_{k+1}, smax(dn, r_{k+1}))
 *                                           : smax(dn, smin(b_{k+1}, r_{k+1})));
 *           tt_{k+1} = tt_k + (2.0*d_k)/smax(1e-6, w_k + w_{k+1}).
 *           A car inside the envelope stays inside it (w_{k+1} <= b_{k+1}), so reachable implies
 *           v_end <= v_target; a car outside brakes as hard as the cfg allows.  A NaN r never
 *           enters w.
 *   per query   stop_node = K_s; reachable (0 or 1); with g_k = smin(b_k, r_k):
 *           overspeed = #{k in [0, K_s] : w_k > g_k}, v_excess = the largest w_k - g_k over the
 *           same k, or 0.0 (serial: e = 0.0, then e = smax(e, w_k - g_k) in index order);
 *           t_stop = tt_{K_s}; v_end = w_{K_s}; s_stop = (double)n_{K_s}*h; brake_node = the
 *           first k in [0, K_s] with b_k < r_k, where the stop starts to bind (none, a target
 *           that is not below the row's speed: K_s).
 *   ticks   tau_m = (double)m*dt, counted from the car.  count = #{m < M_cap : tau_m < tt_{K_s}};
 *           every tick lies on the march: the rejoin stage's node bisection over tt[0..K_s] and
 *           its march-tick columns s, x, y, heading, kappa, v, ax apply unchanged.  Ticks at or
 *           after t_stop are not produced: the caller holds the target state.
 * raceline.stop_host states the same in NumPy; the kernel equals it bit for bit.  These are
 * additions to ABI 6.1 that leave RL_ABI_MINOR as it is: RL_FEATURE_STOP announces them. */
typedef struct rl_stp_query {
    rl_rjn_query   rj;           /* the rejoin stage's query, with the same meaning and checks */
    const int32_t* stop_sample;  /* [Q] row sample J in [0, N) */
    const double*  v_target;     /* [Q] the speed to have at J, finite and >= 0; NULL: all 0.0 */
} rl_stp_query;

typedef struct rl_stp {          /* caller-allocated; NULL fields skipped; it begins as rl_rjn does */
    double *s, *x, *y, *heading, *kappa, *v, *ax;   /* [Q][M_cap]; ticks m >= count[q] are unspecified */
    double *u, *t0, *s0, *e, *dist2;                /* [Q] */
    int32_t *seg, *count;                           /* [Q] */
    int32_t *stop_node, *overspeed;                 /* [Q] */
    double *t_stop, *v_end;                         /* [Q] */
    double *node_v, *node_t;                        /* [Q][K_cap+1] w_k, tt_k; entries past K_s are unspecified;
                                                       downloaded only when asked for */
    int32_t *reachable, *brake_node;                /* [Q] */
    double *s_stop, *v_excess;                      /* [Q] */
    double *node_b;                                 /* [Q][K_cap+1] b_k, as node_v */
} rl_stp;

/* Enqueue the stage after the plan's last trajectory stage: rl_plan_horizon's stream, validity
 * and invalidation rules.  It leaves the results, the trajectory stage and the last horizon and
 * rejoin stages untouched; its buffers are plan-owned (they count toward the plan cache's
 * budget) and grow with Q, M_cap and K_cap.  The query's arrays and cfg are read before the
 * call returns.  rl_plan_kernel_ms index 10 is the stage.  RL_EINVAL before any device work
 * for: every error of rl_plan_rejoin, a NULL stop_sample, a stop_sample[q] outside [0, N), a
 * v_target[q] that is not finite or is < 0. */
int rl_plan_stop(rl_plan* plan, const rl_stp_query* query, void* hip_stream);
/* Download the last stop stage (synchronises its stream) into the non-NULL fields of out.
 * RL_EINVAL before a stage, or after a run or trajectory stage that followed it. */
int rl_plan_fetch_stop(rl_plan* plan, rl_stp* out);
/* The same on B given rows [B][N] with steps h [B] (host in, host out): the trajectory kernel
 * for the stamps, then the stop kernel.  Errors as rl_rejoin's, and the query errors above. */
int rl_stop(const double* x, const double* y, const double* heading, const double* kappa,
            const double* v, const double* ax, const double* h, int32_t N, int32_t B,
            int32_t closed, const rl_stp_query* query, int32_t device, rl_stp* out);

/* ------------------------------------------------- retime stage: the look-ahead speed profile under the car's limits now
 * The rejoin and stop stages follow the row's own speed r, which was computed under the planning
 * cfg; the car's limits now enter their marches only along the path (ax_max_at).  With less grip
 * than the plan had, every corner of r is too fast, and neither stage brakes for a corner ahead.
 * This stage runs the reference's velocity_profile_forward_backward itself over the nodes ahead
 * of the car, with the query's cfg and from the car's speed: the path stays, the speeds are
 * recomputed.  It is what a controller calls when its friction estimate changes.  The query is
 * the rejoin stage's.  In fp64 without contraction; smax, smin, the row, ax_max_at, the march's
 * step and time are the rejoin stage's:
 *   locate, nodes   the rejoin stage's: seg = i, u, e, dist2, t0, s0; kappa_k, r_k, d_k,
 *           n_k = i + k for k = 0..K, K = K_lim = min(K_cap, closed ? N : N-1-i).  A NaN winner,
 *           S = 0, or K_lim < 1 (an open row's last sample): seg as located or -1,
 *           end_node = -1, count = 0, nothing else is specified.
 *   ceiling   per node, independent of the others:
 *           c_k = smin(smin(v_cap_mps, sqrt(a_lat_max / smax(fabs(kappa_k), kappa_eps))), r_k)
 *           with the query's cfg: the reference's initial profile, in its order, capped by the
 *           row's speed.  A NaN r_k does not cap (smin(x, NaN) = x).  r caps on purpose: the
 *           stage never drives the path faster than it was planned for.
 *   envelope   serial, backward: b_K = c_K.  For k = K-1 .. 0:
 *           (., a_brk) = ax_max_at(cfg, b_{k+1}, kappa_{k+1});
 *           b_k = smin(c_k, sqrt(smax(0.0, b_{k+1}*b_{k+1} + (2.0*a_brk)*d_k)))
 *           (the reference's backward step).  feasible = (v0 <= b_0).
 *   march   serial, forward, always to K: w_0 = v0, tt_0 = 0.0.  For k = 0 .. K-1:
 *           (up, dn) = the rejoin march's step from w_k at kappa_k over d_k;
 *           w_{k+1} = smin(up, (w_k <= b_k) ? b_{k+1} : smax(dn, b_{k+1}));
 *           tt_{k+1} = tt_k + (2.0*d_k)/smax(1e-6, w_k + w_{k+1}).
 *           Inside the envelope the envelope caps the speed, as in the stop stage; outside it
 *           the car brakes as hard as the cfg allows.  From v0 = b_0 on a row whose nodes are its
 *           samples, w is the reference's converged profile bit for bit (one backward and one
 *           forward sweep reach its fixed point).
 *   per query   end_node = K; feasible (0 or 1); overspeed = #{k in [0, K] : w_k > b_k};
 *           v_excess = the largest w_k - b_k over the same k, or 0.0 (serial: e = 0.0, then
 *           e = smax(e, w_k - b_k) in index order); bind_node = the first k in [0, K] with
 *           b_k < r_k, where today's limits first fall below the plan (none: -1);
 *           t_end = tt_K; with c0 = floor(n_K / N) and j = n_K - c0*N,
 *           t_loss = tt_K - (((double)c0*T + t[j]) - t0), the time lost against the plan over
 *           the window.
 *   ticks   tau_m = (double)m*dt, counted from the car.  count = #{m < M_cap : tau_m < tt_K};
 *           every tick lies on the march: the rejoin stage's node bisection over tt[0..K] and
 *           its march-tick columns apply unchanged.  The stage never hands over to the row's
 *           own ticks.
 * Known limit: the envelope starts from c_K, so a corner beyond node K is not foreseen.  Callers
 * use the first part of the window and query again.
 * raceline.retime_host states the same in NumPy; the kernel equals it bit for bit.  These are
 * additions to ABI 6.1 that leave RL_ABI_MINOR as it is: RL_FEATURE_RETIME announces them. */
typedef struct rl_rtm_query {
    rl_rjn_query   rj;           /* the rejoin stage's query, with the same meaning and checks */
} rl_rtm_query;

typedef struct rl_rtm {          /* caller-allocated; NULL fields skipped; it begins as rl_rjn does */
    double *s, *x, *y, *heading, *kappa, *v, *ax;   /* [Q][M_cap]; ticks m >= count[q] are unspecified */
    double *u, *t0, *s0, *e, *dist2;                /* [Q] */
    int32_t *seg, *count;                           /* [Q] */
    int32_t *end_node, *overspeed;                  /* [Q] */
    double *t_end, *t_loss;                         /* [Q] */
    double *node_v, *node_t;                        /* [Q][K_cap+1] w_k, tt_k; entries past K are unspecified;
                                                       downloaded only when asked for */
    int32_t *feasible, *bind_node;                  /* [Q] */
    double *v_excess;                               /* [Q] */
    double *node_b, *node_c;                        /* [Q][K_cap+1] b_k, c_k, as node_v */
} rl_rtm;

/* Enqueue the stage after the plan's last trajectory stage: rl_plan_horizon's stream, validity
 * and invalidation rules.  It leaves the results, the trajectory stage and the last horizon,
 * rejoin and stop stages untouched; its buffers are plan-owned (they count toward the plan
 * cache's budget) and grow with Q, M_cap and K_cap.  The query's arrays and cfg are read before
 * the call returns.  rl_plan_kernel_ms index 13 is the stage.  RL_EINVAL before any device work
 * for: every error of rl_plan_rejoin. */
int rl_plan_retime(rl_plan* plan, const rl_rtm_query* query, void* hip_stream);
/* Download the last retime stage (synchronises its stream) into the non-NULL fields of out.
 * RL_EINVAL before a stage, or after a run or trajectory stage that followed it. */
int rl_plan_fetch_retime(rl_plan* plan, rl_rtm* out);
/* The same on B given rows [B][N] with steps h [B] (host in, host out): the trajectory kernel
 * for the stamps, then the retime kernel.  Errors as rl_rejoin's. */
int rl_retime(const double* x, const double* y, const double* heading, const double* kappa,
              const double* v, const double* ax, const double* h, int32_t N, int32_t B,
              int32_t closed, const rl_rtm_query* query, int32_t device, rl_rtm* out);

/* ------------------------------------------------- bounds stage: the free track width along the rows
 * Every tick of the stages above carries s, x, y, heading, kappa, v, ax, and the location carries
 * the lateral offset e.  This stage says how much room there is on either side: an MPC's track
 * constraint at every tick, a tracker's margin for e.  It casts the optimisers' corridor
 * (rl_corridor's device code, the plan's resident rings) about the rows of the last trajectory
 * stage as they lie on the device.  In fp64 without contraction, per row r (the trajectory
 * stage's row r: instance index[r] of a stage over the selected rows) and sample i, with the
 * row's own points P_i = (x_i, y_i):
 *   normal  normals_from_points_generic (ref:581-593): N == 1: t = (1, 0).  Closed rows:
 *           t = (P_{(i+1) mod N} - P_{(i-1) mod N})*0.5.  Open rows: t = P_1 - P_0 at i = 0,
 *           t = P_{N-1} - P_{N-2} at i = N-1, t = (P_{i+1} - P_{i-1})*0.5 between.
 *           sqrt(tx*tx + ty*ty) < 1e-15: t = (1, 0).  v = (-ty, tx), l = sqrt(vx*vx + vy*vy),
 *           (nx, ny) = l < 1e-15 ? (0, 0) : (vx/l, vy/l): +n is left of travel, the sign of the
 *           horizon stage's e.
 *   bounds  guard = veh_width*0.5 + margin; dpos / dneg the safe_ray distances (ref:694-699)
 *           along +n / -n to the nearer ring; hi = max(0, dpos - guard), lo = -max(0, dneg - guard)
 *           (ref:692-711): bit for bit rl_corridor's lo, hi for a problem whose center_xy is the
 *           row, whose veh_width is veh_width and whose cfg.safety_margin_m is margin, zero signs
 *           and empty rings included.
 * At the horizon stage's ticks (rl_plan_horizon_bounds), per query q with seg >= 0 and tick
 * m < count[q]: tau_m = t0 + (double)m*dt, the horizon stage's wrap (c, w) and its bisection on w
 * give the tick's segment i, j = (i + 1) mod N, and with smax(a, b) = a < b ? b : a and
 * smin(a, b) = b < a ? b : a
 *           lo_m = smax(lo_i, lo_j), hi_m = smin(hi_i, hi_j),
 * the conservative pair of the segment's two samples: never looser than either, no rounding.
 * lo0, hi0 are the same pair of the located segment seg: with e, the room now is hi0 - e on the
 * left and e - lo0 on the right.  A query with seg = -1 writes nothing that is specified.  The
 * ticks of the rejoin and stop stages lie on march nodes, node k is sample n_k: rl_bnd's rows
 * serve them as they are.  raceline.normals_host and raceline.horizon_bounds_host state the
 * two new pieces in NumPy.  These are additions to ABI 6.1 that leave RL_ABI_MINOR as it is:
 * RL_FEATURE_BOUNDS announces them. */
typedef struct rl_bnd_query {
    double veh_width;            /* finite */
    double margin;               /* finite */
} rl_bnd_query;

typedef struct rl_bnd {          /* caller-allocated; NULL fields skipped */
    double *lo, *hi, *nx, *ny;   /* [R][N] */
} rl_bnd;

typedef struct rl_hzn_bnd {      /* caller-allocated; NULL fields skipped */
    double *lo, *hi;             /* [Q][M_cap]; ticks m >= count[q] are unspecified */
    double *lo0, *hi0;           /* [Q] */
} rl_hzn_bnd;

/* Enqueue the stage after the plan's last trajectory stage: rl_plan_horizon's stream, validity
 * and invalidation rules.  Bounds row r is trajectory row r for every later query.  It leaves
 * the results, the trajectory stage and the horizon, rejoin and stop stages untouched; its
 * buffers are plan-owned (they count toward the plan cache's budget) and grow with R.
 * rl_plan_kernel_ms index 11 is the stage.  RL_EINVAL before any device work for: a NULL plan or
 * query, a veh_width or margin that is not finite, no valid trajectory stage. */
int rl_plan_bounds(rl_plan* plan, const rl_bnd_query* query, void* hip_stream);
/* Download the last bounds stage (synchronises its stream) into the non-NULL fields of out.
 * RL_EINVAL before a stage, or after a run or trajectory stage that followed it. */
int rl_plan_fetch_bounds(rl_plan* plan, rl_bnd* out);
/* Enqueue the bounds at the ticks of the last horizon stage; it reads that stage's row, seg, t0
 * and count and the bounds stage's rows on the device and uploads nothing.  RL_EINVAL unless a
 * valid horizon stage and a valid bounds stage follow the same trajectory stage.  A later
 * horizon or bounds stage needs another call.  rl_plan_kernel_ms index 12 is the stage. */
int rl_plan_horizon_bounds(rl_plan* plan, void* hip_stream);
/* Download the last rl_plan_horizon_bounds (synchronises its stream) into the non-NULL fields of
 * out, Q and M_cap the horizon stage's.  RL_EINVAL before one, or after a run, a trajectory,
 * horizon or bounds stage that followed it. */
int rl_plan_fetch_horizon_bounds(rl_plan* plan, rl_hzn_bnd* out);
/* The same bounds for B given rows x, y [B][N] (host in, host out).  The rings, N and closed
 * are prob's; prob->center_xy, L and veh_width are not read.  The rings are uploaded once for
 * all rows.  RL_EINVAL before any device work for: a NULL prob, x, y or out, B < 1, N < 0, bad
 * segments, a veh_width or margin that is not finite; RL_ETOOBIG for N > 1048576. */
int rl_bounds(const rl_problem* prob, const double* x, const double* y, int32_t B, double veh_width,
              double margin, int32_t device, rl_bnd* out);

/* ------------------------------------------------- recover stage: a path from the car's offset back to the raceline
 * Every stage above serves ticks whose x, y lie on the row: a car that is off the line by e gets
 * ticks that start e to its side.  This stage serves the path back: a lateral offset profile from
 * the car's e (and heading error) to zero over a merge length, kept inside the free width of the
 * last bounds stage, the geometry of that offset path, the retime stage's speed pass on that
 * geometry, and the ticks along it.  In fp64 without contraction; smax, smin, the row,
 * ax_max_at, the march's step and time are the rejoin stage's:
 *   locate, nodes   the rejoin stage's: seg = i, u, e, dist2, t0, s0; kappa_k, r_k, d_k,
 *           n_k = i + k for k = 0..K, K = K_lim = min(K_cap, closed ? N : N-1-i), K_cap in
 *           1..RL_RCV_MAX_NODES.  A NaN winner, S = 0 or K < 1: seg as located or -1,
 *           end_node = -1, count = 0, nothing else is specified.  The stage reads the last
 *           bounds stage's lo, hi, nx, ny of the query's row (below: at row index n_k mod N);
 *           j = (i+1) mod N.
 *   slope   dir_xy [Q][2] (optional): the car's direction of travel (hx, hy), finite, any length.
 *           With (dx, dy) the located segment's direction P_j - P_i:
 *           den = dx*hx + dy*hy, num = dx*hy - dy*hx,
 *           g0 = den > 0 ? smin(1.0, smax(-1.0, num/den)) : (num < 0 ? -1.0 : (num > 0 ? 1.0 : 0.0)):
 *           de/ds, capped at 45 degrees, without trigonometry.  dir_xy == NULL: g0 = 0.0.
 *   offsets   D = merge_len[q], finite and > 0.  a_0 = 0.0, a_k = d_0 + (double)(k-1)*h,
 *           z_k = smin(1.0, a_k / D), z3 = (z*z)*z,
 *           qz = 1.0 + z3*(-10.0 + z*(15.0 - 6.0*z)), pz = z + z3*(-6.0 + z*(8.0 - 3.0*z)).
 *           o_0 = e; for k >= 1: o_k = smin(hi_{n_k}, smax(lo_{n_k}, e*qz + (g0*D)*pz)): the
 *           quintic with value e, slope g0 and no second derivative at the car and value, slope
 *           and second derivative zero at D, clamped to the free width.  At z = 1 both
 *           polynomials are exactly 0.  clamped = #{k in [1, K] : the clamp changed the value};
 *           offtrack = !(lo0 <= e && e <= hi0) with lo0 = smax(lo_i, lo_j), hi0 = smin(hi_i, hi_j);
 *           merge_node = the first k with z_k >= 1.0 (none in [0, K]: -1).
 *   points   P_0 = (X0 + rx, Y0 + ry): (X0, Y0) the rejoin stage's node 0, (rx, ry) the locate's
 *           residual (wx - u*dx, wy - u*dy).  P_k = (x_{n_k} + o_k*nx_{n_k}, y_{n_k} + o_k*ny_{n_k})
 *           for k >= 1.
 *   geometry   Segment k is on the line if o_k == 0.0 && o_{k+1} == 0.0: d'_k = d_k.  Otherwise
 *           d'_k = sqrt(qx*qx + qy*qy), q = P_{k+1} - P_k.  Node k is on the line if o_m == 0.0
 *           for every m of {k-1, k, k+1} within [0, K]: kappa'_k = kappa_k and psi_k is the rejoin
 *           stage's node heading.  Otherwise, for 1 <= k <= K-1 with a = P_k - P_{k-1},
 *           b = P_{k+1} - P_k, c = P_{k+1} - P_{k-1}: den = (d'_{k-1}*d'_k)*sqrt(cx*cx + cy*cy),
 *           kappa'_k = den > 0 ? (2.0*(ax*by - ay*bx))/den : 0.0 (Menger), psi_k = atan2_cr(cy, cx).
 *           End nodes off the line: kappa'_0 = kappa'_1 and kappa'_K = kappa'_{K-1} when K >= 2,
 *           otherwise the row's; psi_0 = atan2_cr of P_1 - P_0, psi_K = atan2_cr of P_K - P_{K-1}.
 *   ceiling, envelope, march, per query   the retime stage's, word for word, with kappa'_k for
 *           kappa_k and d'_k for d_k: c_k, b_k, feasible, w_k, tt_k, overspeed, v_excess,
 *           bind_node, end_node = K, t_end, t_loss.
 *   ticks   tau_m = (double)m*dt.  count = #{m < M_cap : tau_m < tt_K}.  The rejoin stage's node
 *           bisection over tt[0..K] gives k and u_m; x, y between P_k and P_{k+1}; heading along
 *           the shorter arc between psi_k and psi_{k+1}; kappa between kappa'_k and kappa'_{k+1};
 *           v and ax the march-tick expressions with d'_k; s = s_k + u_m*(s_{k+1} - s_k), the
 *           station along the raceline as in the rejoin stage; offset = o_k + u_m*(o_{k+1} - o_k).
 *           The stage never hands over to the row's own ticks.
 * Anchor: a pose with e == 0.0 and g0 == 0.0 has every o_k == 0.0, every node and segment is on
 * the line, and the stage is the retime stage bit for bit with offset all zeros.
 * Known limits: the window ends at node K like the retime stage's, so a corner or the rest of the
 * merge beyond node K is not foreseen.  A car far off the line with u near 1 gets a short, sharp
 * first segment and is reported feasible = 0; it is not rescued.
 * raceline.recover_host states the same in NumPy; the kernel equals it bit for bit except in
 * heading where a node is off the line (atan2_cr is correctly rounded).  These are additions to
 * ABI 6.1 that leave RL_ABI_MINOR as it is: RL_FEATURE_RECOVER announces them. */
#define RL_RCV_MAX_NODES 512
typedef struct rl_rcv_query {
    rl_rjn_query   rj;           /* the rejoin stage's query; K_cap in 1..RL_RCV_MAX_NODES */
    const double*  merge_len;    /* [Q] D, finite and > 0 */
    const double*  dir_xy;       /* [Q][2] the car's direction of travel, finite; NULL: g0 = 0.0 */
} rl_rcv_query;

typedef struct rl_rcv {          /* caller-allocated; NULL fields skipped; it begins as rl_rtm does */
    double *s, *x, *y, *heading, *kappa, *v, *ax;   /* [Q][M_cap]; ticks m >= count[q] are unspecified */
    double *u, *t0, *s0, *e, *dist2;                /* [Q] */
    int32_t *seg, *count;                           /* [Q] */
    int32_t *end_node, *overspeed;                  /* [Q] */
    double *t_end, *t_loss;                         /* [Q] */
    double *node_v, *node_t;                        /* [Q][K_cap+1] w_k, tt_k; entries past K are unspecified;
                                                       downloaded only when asked for */
    int32_t *feasible, *bind_node;                  /* [Q] */
    double *v_excess;                               /* [Q] */
    double *node_b, *node_c;                        /* [Q][K_cap+1] b_k, c_k, as node_v */
    double *offset;                                 /* [Q][M_cap] as the columns */
    int32_t *clamped, *offtrack;                    /* [Q] */
    int32_t *merge_node;                            /* [Q] */
    double *lo0, *hi0;                              /* [Q] */
    double *node_o, *node_k;                        /* [Q][K_cap+1] o_k, kappa'_k, as node_v */
} rl_rcv;

/* Enqueue the stage after the plan's last trajectory and bounds stages: rl_plan_retime's stream,
 * validity and invalidation rules, and a later bounds stage invalidates it as well.  It leaves
 * the results, the trajectory stage and the last horizon, rejoin, stop, retime and bounds stages
 * untouched; its buffers are plan-owned (they count toward the plan cache's budget) and grow with
 * Q, M_cap and K_cap.  The query's arrays and cfg are read before the call returns.
 * rl_plan_kernel_ms index 14 is the stage.  RL_EINVAL before any device work for: every error of
 * rl_plan_retime, K_cap > RL_RCV_MAX_NODES, a NULL merge_len, a merge_len[q] that is not finite
 * or is <= 0, a dir_xy that is not finite, no valid bounds stage after the trajectory stage. */
int rl_plan_recover(rl_plan* plan, const rl_rcv_query* query, void* hip_stream);
/* Download the last recover stage (synchronises its stream) into the non-NULL fields of out.
 * RL_EINVAL before a stage, or after a run, a trajectory or a bounds stage that followed it. */
int rl_plan_fetch_recover(rl_plan* plan, rl_rcv* out);
/* The same on B given rows [B][N] with steps h [B] and their bounds lo, hi, nx, ny [B][N] (host
 * in, host out): the trajectory kernel for the stamps, then the recover kernel.  Errors as
 * rl_retime's and rl_plan_recover's, and a NULL lo, hi, nx or ny. */
int rl_recover(const double* x, const double* y, const double* heading, const double* kappa,
               const double* v, const double* ax, const double* h, const double* lo, const double* hi,
               const double* nx, const double* ny, int32_t N, int32_t B, int32_t closed,
               const rl_rcv_query* query, int32_t device, rl_rcv* out);

/* ------------------------------------------------- fan stage: several merge lengths per pose, the best one served
 * The recover stage's caller chooses merge_len before knowing what it costs: feasible, clamped,
 * merge_node and t_end are known only after the stage has run.  This stage evaluates C merge
 * lengths for each pose on the device, ranks them in an exact order and serves the winner's
 * results with a small table of every candidate's per-query values.
 *   query   the recover stage's, with merge_len [Q][C], C = n_cand in 1..RL_FAN_MAX_CAND, K_cap in
 *           1..RL_RCV_MAX_NODES, Q*C <= RL_HZN_MAX_QUERIES, every merge_len[q][c] finite and > 0;
 *           duplicate lengths are allowed.
 *   candidates   candidate c of query q is the recover stage's answer for query q with
 *           D = merge_len[q][c], word for word.  All candidates of a query share the locate (seg,
 *           u, e, dist2, t0, s0), K, lo0, hi0 and offtrack.
 *   class   g = 0: feasible && clamped == 0 && merge_node >= 0; g = 1: feasible && merge_node >= 0;
 *           g = 2: feasible; g = 3: otherwise.
 *   order   ascending in (g, isnan(t_end), t_end, c), with plain < on doubles and no tolerance;
 *           best[q] is the first candidate in that order: the path that is drivable from the car's
 *           speed, was not cut by the track's edge and is on the row again inside the window; among
 *           such paths the one that reaches node K soonest, and the earlier candidate on a tie.
 *   empty   a query that the recover stage answers with end_node = -1 has best = -1; seg, count = 0
 *           and end_node = -1 are as the recover stage specifies them, nothing else is specified.
 *   results   every field of rl_rcv, holding the winner's values (the node arrays downloaded only
 *           when asked for), then best [Q] and the table [Q][C].  Losers' ticks and node arrays
 *           never leave the device.
 * Anchors: with C = 1 the stage is the recover stage bit for bit.  For any C the winner's fields
 * equal rl_recover's for merge_len[q][best[q]] bit for bit, heading included, and table row c equals
 * the per-query values of rl_recover with merge_len[q][c].  A pose on the row with g0 == 0 has
 * equal t_end for every D, so best = 0 except where a class differs through merge_node.
 * raceline.recover_fan_host states the same in NumPy (recover_host C times, then
 * raceline.fan_order).  These are additions to ABI 6.1 that leave RL_ABI_MINOR as it is:
 * RL_FEATURE_FAN announces them. */
#define RL_FAN_MAX_CAND 16
typedef struct rl_fan_query {
    rl_rcv_query   rc;           /* the recover stage's query, its merge_len [Q][n_cand] */
    int32_t        n_cand;       /* C, 1..RL_FAN_MAX_CAND; Q*C <= RL_HZN_MAX_QUERIES */
    int32_t        _pad;
} rl_fan_query;

typedef struct rl_fan {          /* caller-allocated; NULL fields skipped; it begins as rl_rcv does */
    double *s, *x, *y, *heading, *kappa, *v, *ax;   /* [Q][M_cap]; ticks m >= count[q] are unspecified */
    double *u, *t0, *s0, *e, *dist2;                /* [Q] */
    int32_t *seg, *count;                           /* [Q] */
    int32_t *end_node, *overspeed;                  /* [Q] */
    double *t_end, *t_loss;                         /* [Q] */
    double *node_v, *node_t;                        /* [Q][K_cap+1] as rl_rcv's; downloaded only when asked for */
    int32_t *feasible, *bind_node;                  /* [Q] */
    double *v_excess;                               /* [Q] */
    double *node_b, *node_c;                        /* [Q][K_cap+1] as node_v */
    double *offset;                                 /* [Q][M_cap] as the columns */
    int32_t *clamped, *offtrack;                    /* [Q] */
    int32_t *merge_node;                            /* [Q] */
    double *lo0, *hi0;                              /* [Q] */
    double *node_o, *node_k;                        /* [Q][K_cap+1] as node_v */
    int32_t *best;                                  /* [Q] the winner's c; -1: an empty query */
    int32_t *cand_class, *cand_feasible, *cand_clamped, *cand_merge_node, *cand_overspeed,
            *cand_bind_node;                        /* [Q][C] */
    double *cand_t_end, *cand_t_loss, *cand_v_excess;   /* [Q][C] */
} rl_fan;

/* Enqueue the stage after the plan's last trajectory and bounds stages: rl_plan_recover's stream,
 * validity and invalidation rules (a later run, trajectory or bounds stage invalidates it).  It
 * leaves the results, the trajectory stage and the last horizon, rejoin, stop, retime, recover and
 * bounds stages untouched; its buffers, the candidates' scratch block among them, are plan-owned
 * (they count toward the plan cache's budget) and grow with Q, C, M_cap and K_cap.  The query's
 * arrays and cfg are read before the call returns.  rl_plan_kernel_ms index 15 is the stage (both
 * kernels).  RL_EINVAL before any device work for: every error of rl_plan_recover, n_cand outside
 * 1..RL_FAN_MAX_CAND, Q*n_cand > RL_HZN_MAX_QUERIES, a merge_len[q][c] that is not finite or is <= 0. */
int rl_plan_recover_fan(rl_plan* plan, const rl_fan_query* query, void* hip_stream);
/* Download the last fan stage (synchronises its stream) into the non-NULL fields of out.
 * RL_EINVAL before a stage, or after a run, a trajectory or a bounds stage that followed it. */
int rl_plan_fetch_recover_fan(rl_plan* plan, rl_fan* out);
/* The same on B given rows and their bounds, as rl_recover.  Errors as rl_recover's and
 * rl_plan_recover_fan's. */
int rl_recover_fan(const double* x, const double* y, const double* heading, const double* kappa,
                   const double* v, const double* ax, const double* h, const double* lo, const double* hi,
                   const double* nx, const double* ny, int32_t N, int32_t B, int32_t closed,
                   const rl_fan_query* query, int32_t device, rl_fan* out);

/* ------------------------------------------------- rollout stage: sampled trajectories scored against the plan
 * Every stage above is interpolated from the raceline and its speed profile; none can judge a
 * trajectory the controller proposes itself.  A sampling controller (MPPI, a lattice planner, a
 * learned policy's candidates) proposes a few thousand short rollouts at every step.  This stage
 * locates each rollout's poses on a row of the last trajectory stage, pose t next to pose t-1, and
 * returns per rollout how far along the line it gets, how far off it strays, whether it leaves the
 * last bounds stage's free width, how its speed compares with the row's, one cost, and the best
 * rollouts of every group.  In fp64 without contraction; smax, smin, the row, its S segments and
 * its step h are the horizon stage's:
 *   query   Q rollouts of T poses: xy [Q][T][2], optional speeds v [Q][T], row [Q] (NULL: 0),
 *           seg_hint [Q] >= -1 for pose 0 (NULL: -1, every segment; a hint past the row is allowed).
 *           1 <= Q <= RL_RLL_MAX_ROLLOUTS, 1 <= T <= RL_RLL_MAX_STEPS, Q*T <= RL_RLL_MAX_POSES.
 *   chain   pose 0 is located exactly as the horizon stage locates a pose with hint seg_hint and
 *           window window0; pose t >= 1 with hint seg_{t-1} and window `window`: the same candidates
 *           (every segment of a closed row when 2W + 1 >= S; none for a hint past an open row), the
 *           same distance D, the same least (isnan(D), D, i).  Per pose: seg, u, dist2 = D and e as
 *           the horizon stage's location.  The chain ends at the first pose without a winner (a NaN
 *           winner, or no candidate): count = t, the per-pose values from t on are NaN and seg -1,
 *           valid = 0, progress = cost = NaN.  A row without a segment: count = 0.
 *   progress   c_0 = 0; for t >= 1 on a closed row with d = seg_t - seg_{t-1}: c_t = c_{t-1} + 1 if
 *           2d < -S, c_{t-1} - 1 if 2d > S, c_{t-1} otherwise; on an open row c_t = 0.
 *           s_t = (((double)c_t*(double)S + (double)seg_t) + u_t)*h; progress = s_{T-1} - s_0.
 *   room    i = seg_t, j = (i+1) mod N: lo_t = smax(lo_i, lo_j), hi_t = smin(hi_i, hi_j) of the bounds
 *           rows (rl_hzn_bnd's pair); margin_t = smin(hi_t - e_t, e_t - lo_t).
 *   speed   vref_t = v_i + u_t*(v_j - v_i) of the row.
 *   per rollout   over the located poses t < count, in ascending t, every sum started from 0.0:
 *           E = sum e_t*e_t, O = sum (margin_t < 0 ? margin_t*margin_t : 0.0),
 *           V = sum (v_t - vref_t)*(v_t - vref_t) (0.0 when v is NULL); e_max = smax(e_max, |e_t|) from
 *           0.0; margin_min = smin(margin_min, margin_t) from +inf; first_out = the first t with
 *           margin_t < 0 (none: T).  valid = (count == T), and then
 *           cost = ((w_e*E + w_out*O) + w_v*V) - w_prog*progress, replaced by +inf if hard_bounds is
 *           set and first_out < T.
 *   ranking   order [G][k], G = Q/group_size (group_size 0: Q), 1 <= k <= min(group_size,
 *           RL_SELECT_MAX_K): the global indices of the k best rollouts of each group, ascending in
 *           (isnan(cost), cost, index): rl_rank_scores' order on cost, by its kernel.
 * raceline.rollouts_host states the same in NumPy; the kernel equals it bit for bit.  These are
 * additions to ABI 6.1 that leave RL_ABI_MINOR as it is: RL_FEATURE_ROLLOUT announces them. */
#define RL_RLL_MAX_ROLLOUTS 65536
#define RL_RLL_MAX_STEPS 512
#define RL_RLL_MAX_POSES (1 << 22)
typedef struct rl_rll_query {
    const double*  xy;           /* [Q][T][2] */
    const double*  v;            /* [Q][T] the rollouts' speeds; NULL: no speed term */
    const int32_t* row;          /* [Q] row of the trajectory stage; NULL: 0 */
    const int32_t* seg_hint;     /* [Q] hint of pose 0, >= -1; NULL: -1 */
    int32_t        Q, T;
    int32_t        window0;      /* >= 0, used with seg_hint for pose 0 */
    int32_t        window;       /* >= 0, used for poses t >= 1 */
    double         w_e, w_out, w_v, w_prog;   /* each finite and >= 0 */
    int32_t        hard_bounds;  /* 0 / 1 */
    int32_t        group_size;   /* 0: Q; Q is a multiple of it */
    int32_t        k;            /* 1..min(group_size, RL_SELECT_MAX_K) */
    int32_t        _pad;
} rl_rll_query;

typedef struct rl_rll {          /* caller-allocated; NULL fields skipped */
    int32_t *seg;                                   /* [Q][T] */
    double *u, *e, *dist2, *s, *margin, *vref;      /* [Q][T]; downloaded only when asked for, as seg */
    int32_t *count, *valid, *first_out;             /* [Q] */
    double *progress, *e_max, *margin_min, *cost;   /* [Q] */
    int32_t *order;                                 /* [G][k] */
} rl_rll;

/* Enqueue the stage after the plan's last trajectory and bounds stages: rl_plan_recover's stream,
 * validity and invalidation rules (a later run, trajectory or bounds stage invalidates it).  It
 * leaves the results and every other stage untouched; its buffers are plan-owned (they count toward
 * the plan cache's budget) and grow with Q*T.  The query's arrays are read before the call returns.
 * rl_plan_kernel_ms index 16 is the stage (locate and rank together).  RL_EINVAL before any device
 * work for: a NULL plan, query or xy; no valid trajectory stage, or no valid bounds stage after it;
 * Q, T or Q*T out of range; a negative window; a weight that is not finite or is < 0; a row outside
 * the trajectory stage's [0, R); a seg_hint < -1; Q not a multiple of group_size; k out of range. */
int rl_plan_rollouts(rl_plan* plan, const rl_rll_query* query, void* hip_stream);
/* Download the last rollout stage (synchronises its stream) into the non-NULL fields of results:
 * the per-rollout values and order always, the per-pose arrays only when results asks for one.
 * RL_EINVAL before a stage, or after a run, a trajectory or a bounds stage that followed it. */
int rl_plan_fetch_rollouts(rl_plan* plan, rl_rll* results);
/* The same on B given rows [B][N] with steps h [B] and their bounds rows lo, hi [B][N] (host in,
 * host out); `row` counts the given rows.  Of the rows the stage reads x, y and v; heading, kappa
 * and ax are taken for the other one-shots' sake.  Errors as rl_plan_rollouts', and a NULL row, h,
 * lo, hi or results, B < 1, N < 1; RL_ETOOBIG for N > 1048576. */
int rl_rollouts(const double* x, const double* y, const double* heading, const double* kappa,
                const double* v, const double* ax, const double* h, const double* lo, const double* hi,
                int32_t N, int32_t B, int32_t closed, const rl_rll_query* query, int32_t device,
                rl_rll* results);

/* B lap evaluations of given paths: heading/curvature
 * (heading_curv_from_points_generic, ref:595-620) and velocity_profile_forward_backward
 * (ref:782-862) with h = L[b]/N on path b — the min-time driver's final step
 * (ref:1045-1048) and the debug dump's centreline / min-curvature laps (ref:1466-1478),
 * i.e. compute_min_time_raceline with max_outer_iters = 0.  paths_xy [B][N][2], L [B];
 * `out` receives heading, kappa, v, ax, lap and vpass_sweeps [B][1] (x, y echo the path,
 * alphas are 0); evals/accepts may be NULL.  cfg[n_cfg] as in rl_optimize.
 * *kernel_ms (optional): HIP-event time of the kernel. */
int rl_lap_eval(const double* paths_xy, const double* L, int32_t N, int32_t B, int32_t closed,
                const rl_cfg* cfg, int32_t n_cfg, int32_t device, rl_out* out, float* kernel_ms);

/* ------------------------------------------------------- step 6: geometry
 * pipeline::compute_geom_and_save (ref:1295-1335), the rows of <base>_with_geom.csv:
 * the centreline spline evaluated at s_k = s0 + L*(k/denomN), heading, curvature,
 * ray distances to the rings along ±n (distancesToRings, ref:513-524), width and
 * v_kappa.  SURVEY §8f row 1. */

/* centerline::Spline1D (ref:403-446): knots s[n], coefficients a,b,c,d [n] */
typedef struct rl_spline {
    const double* s;
    const double* a;
    const double* b;
    const double* c;
    const double* d;
    int32_t n;
    int32_t _pad;
} rl_spline;

typedef struct rl_geom_problem {
    rl_spline spx, spy;          /* x(s), y(s) from splineUniformResample (ref:448-474)      */
    double s0, L;                /* resample origin and length (ref:465)                      */
    int32_t Kmax;                /* rows before the duplicate: closed ? samples : Ncenter (ref:1308) */
    int32_t denomN;              /* closed ? samples : max(1, samples) (ref:1309)             */
    int32_t emit_closed_duplicate; /* cfg emit_closed_duplicate: one more row (L, row 0) (ref:1331) */
    int32_t closed;              /* ring segments are ringEdges (1) / polylineEdges (0) inputs */
    const double* inner_seg;     /* [Ei][4] */
    const double* outer_seg;     /* [Eo][4] */
    int32_t Ei, Eo;
} rl_geom_problem;

#define RL_GEOM_COLS 9           /* s_rel,x,y,heading_rad,curvature,dist_to_inner,dist_to_outer,width,v_kappa_mps */

/* Rows (Kmax + emit_closed_duplicate) x RL_GEOM_COLS into host `rows` (row-major),
 * computed on `device`.  cfg supplies kappa_eps, a_lat_max, v_cap_mps.  *kernel_ms
 * (optional) receives the HIP-event time of the geometry kernel.  Returns the row
 * count or RL_E*. */
int rl_geom(const rl_geom_problem* gp, const rl_cfg* cfg, int32_t device, double* rows, float* kernel_ms);

/* ------------------------------------------------------ CSV number format
 * SURVEY §8f row 3.  The reference writes every CSV with std::fixed + precision(9)
 * (ref:1284, 1303, 1354, 1418, 1495), i.e. glibc "%.9f": exact value rounded to 9
 * fraction digits with ties to even, "-" whenever the sign bit is set, "nan"/"-nan",
 * "inf"/"-inf".  rl_format_csv formats a row-major table [rows][cols] on the GPU into
 * `out` as "v,v,...,v\n" rows (no header).  *out_len receives the byte count (also when
 * out_cap is too small: then RL_ETOOBIG); row_offsets [rows+1] (optional) the start of
 * every row.  Values with |x| >= 9.2e9 are rejected (RL_ETOOBIG). */
int rl_format_csv(const double* table, int64_t rows, int32_t cols, int32_t device, char* out, int64_t out_cap,
                  int64_t* out_len, int64_t* row_offsets);

/* ------------------------------------------------------------ corridor
 * The optimisers' first corridor (ref:692-711) for the path prob->center_xy:
 * normals_from_points_generic (ref:581-593), then per sample
 *   hi = max(0, dpos - guard), lo = -max(0, dneg - guard),
 *   guard = prob->veh_width*0.5 + cfg->safety_margin_m,
 * dpos / dneg the safe_ray distances (ref:694-699) along +n / -n to the nearer ring.
 * The same device code as the optimiser's corridor passes (rl_corridor.h), run in
 * the optimiser's scan mapping.  lo, hi: [N] host buffers.  Returns RL_OK or RL_E*. */
int rl_corridor(const rl_problem* prob, const rl_cfg* cfg, int32_t device, double* lo, double* hi);

/* ------------------------------------------------------------- runtime */
int         rl_device_count(void);
const char* rl_last_error(void);
int         rl_abi_version(void);
int         rl_abi_minor(void);
/* additions since the last minor, one bit each (a library without this function has none) */
#define RL_FEATURE_TRAJECTORY 1   /* bit 0: the trajectory stage */
#define RL_FEATURE_HORIZON 2      /* bit 1: the horizon stage */
#define RL_FEATURE_REJOIN 4       /* bit 2: the rejoin stage */
#define RL_FEATURE_STOP 8         /* bit 3: the stop stage */
#define RL_FEATURE_BOUNDS 16      /* bit 4: the bounds stage */
#define RL_FEATURE_RETIME 32      /* bit 5: the retime stage */
#define RL_FEATURE_RECOVER 64     /* bit 6: the recover stage */
#define RL_FEATURE_FAN 128        /* bit 7: the fan stage */
#define RL_FEATURE_ROLLOUT 256    /* bit 8: the rollout stage */
int         rl_abi_features(void);
/* samples per lane of the THROUGHPUT shape for N (4: N <= 256, 5: N <= 320, 8: N <= 4096;
 * 1 = the streaming kernel), or RL_ETOOBIG.  Batches small enough for a latency shape launch fewer samples per lane:
 * rl_kernel_shape(N, B, mode) reports the shape a launch actually uses. */
int         rl_kernel_variant(int32_t N);
/* the kernel shape of a launch: *K samples per lane (0 = the streaming kernel) and *T lanes
 * per instance for N samples, a batch of B and mode RL_MODE_MINCURV or RL_MODE_MINTIME on
 * the calling thread's current device.  Batches that need at most one wave per SIMD in a
 * latency shape (one instance spread over a CU, 1-4 samples per lane) get it; larger ones
 * the throughput shapes (4-8 samples per lane).  RL_LAT_SHAPES=0 in the environment keeps
 * the throughput shapes for every batch.  Returns RL_OK or RL_E*. */
int         rl_kernel_shape(int32_t N, int32_t B, int32_t mode, int32_t* K, int32_t* T);

#ifdef __cplusplus
}
#endif
#endif /* RL_ABI_H */
