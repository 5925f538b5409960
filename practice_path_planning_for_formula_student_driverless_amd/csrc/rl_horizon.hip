// rl_horizon.hip — the horizon stage's kernel: a controller's question, "I am at
// (px, py); where on the raceline is that, and what are the next M ticks from there?", answered
// for Q poses on rows of the last trajectory stage (rl_trajectory.hip, §3k), whose samples,
// step h, stamps t_0 .. t_N and T = t_S it reads as they lie in HBM.  Per query, in fp64
// without contraction (S = closed ? N : N - 1 segments, segment i from sample i to j = (i + 1) mod N):
//     candidates: every i in [0, S) without a hint; with a hint g and window W the segments
//         (g + k) mod S, k = -W .. W, of a closed row (all of them if 2W + 1 >= S), and
//         max(0, g - W) .. min(S - 1, g + W) of an open one
//     distance: dx = x_j - x_i, dy = y_j - y_i, wx = px - x_i, wy = py - y_i, dd = dx*dx + dy*dy,
//         c = wx*dx + wy*dy, u = dd > 0 ? smin(1, smax(0, c/dd)) : 0, rx = wx - u*dx,
//         ry = wy - u*dy, D = rx*rx + ry*ry
//     winner: the candidate least in (isnan(D), D, i); a NaN winner or S = 0: seg = -1, count = 0
//     location: seg = i, u, dist2 = D, e = (dx*wy - dy*wx) < 0 ? -sqrt(D) : sqrt(D),
//         t0 = t_i + u*(t_{i+1} - t_i), s0 = ((double)i + u)*h
//     ticks: tau_m = t0 + (double)m*dt.  Open rows: count = min(M_cap, #{m : tau_m < T}), c = 0,
//         w = tau_m.  Closed rows: count = M_cap if T is finite and > 0, else 0; c = floor(tau_m/T),
//         w = tau_m - c*T, then at most one fix-up each way (w < 0: w += T, c -= 1; else
//         w >= T: w -= T, c += 1).  Segment of a tick: §3k's bisection on w; u_m = (w - t_i) /
//         (t_{i+1} - t_i); s = ((c*(double)S + (double)i) + u_m)*h; the other six columns are §3k's.
// raceline.horizon_host states the same in NumPy, and the two agree bit for bit: each D depends
// on its own segment only, so the shape of the reduction does not show in the result.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_horizon.h"

namespace rl {

// One workgroup per query.  The lanes stride over the candidates and each keeps its least
// (key, index); the wave folds its 64 with an xor butterfly, the waves meet in LDS and every
// lane reads all slots (rl_rank_kernel's scheme).  The same barrier publishes the stamps of a
// row of N <= TRAJ_LDS_N samples, which the lanes copied into LDS on the way; longer rows read
// the trajectory stage's global row.  Lane 0 computes the location and the tick count and hands
// t0 and the count over through LDS; then all lanes stride over m (consecutive lanes,
// consecutive ticks).  No atomics: every output element has one writer.
__global__ __launch_bounds__(HZN_THREADS) void rl_horizon_kernel(HznParams p) {
    __shared__ double s_t[TRAJ_LDS_N + 1];
    __shared__ uint64_t s_key[HZN_THREADS / 64];
    __shared__ uint32_t s_idx[HZN_THREADS / 64];
    __shared__ double s_t0;
    __shared__ int s_count;
    const TrajParams& q = p.src;
    const int k = blockIdx.x, tid = threadIdx.x, N = q.N;
    const int S = q.closed ? N : N - 1;
    const int r = p.row ? p.row[k] : 0, b = hzn_instance(q, r);
    if (b < 0 || b >= q.B || S < 1) {             // no row, or a row without a segment
        if (tid == 0) hzn_empty(p, k);
        return;
    }
    // x and y for the locate; the other four rows are formed where the ticks need them
    const size_t off = (size_t)b * (size_t)N;
    const double *x = q.x + off, *y = q.y + off, *tg = hzn_stamps(q, r);
    const bool lds = N <= TRAJ_LDS_N;
    if (lds)
        for (int i = tid; i <= N; i += HZN_THREADS) s_t[i] = tg[i];
    const double px = p.pose[2 * (size_t)k], py = p.pose[2 * (size_t)k + 1];

    const HznWin win = hzn_locate(p, k, tid, x, y, px, py, s_key, s_idx);
    if (win.key >= HZN_KEY_NAN || win.idx >= (uint32_t)S) {  // a NaN winner, or no candidate at all
        if (tid == 0) hzn_empty(p, k);
        return;
    }
    auto stamp = [&](int i) { return lds ? s_t[i] : tg[i]; };
    const double h = hzn_step(q, b);
    const double T = q.T[r];
    if (tid == 0) {                                // only lane 0 needs the located point: the ticks start from s_t0
        const int i = (int)win.idx;
        const Foot f = hzn_foot(x, y, N, i, px, py);
        const double t0 = hzn_t0(stamp, i, f.u);
        int cnt;
        if (!q.closed) cnt = tick_end(0, p.M_cap, [&](int m) { return t0 + (double)m * p.dt < T; });
        else cnt = (__builtin_isfinite(T) && T > 0.0) ? p.M_cap : 0;
        hzn_store_loc(p, k, f, i, h, t0, cnt);
        s_t0 = t0;
        s_count = cnt;
    }
    __syncthreads();
    const double t0 = s_t0;
    const int M = s_count;
    const HznRow row{x, y, q.heading + off, q.kappa + off, q.v + off, q.ax + off};
    const size_t orow = (size_t)k * (size_t)p.M_cap;
    for (int m = tid; m < M; m += HZN_THREADS) {
        const HznLap l = hzn_wrap(q.closed, T, t0 + (double)m * p.dt);
        hzn_columns(p, row, stamp, N, S, h, l.c, l.w, orow + m);
    }
}

hipError_t launch_horizon(const HznParams& p, hipStream_t st) {
    hipLaunchKernelGGL(rl_horizon_kernel, dim3((unsigned)p.Q), dim3(HZN_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace rl
