// rl_rejoin.hip — the rejoin stage's kernel: "I am at (px, py) doing v0, with these
// limits: what can I drive for the next M ticks, where do I rejoin the plan, and what did that
// cost?"  The horizon stage's query (rl_horizon.hip, §3l) with a speed and one rl_cfg.  Per
// query, in fp64 without contraction:
//     locate: §3l's candidates, distance, winner and location: seg = i, u, e, dist2, t0, s0
//     nodes: node 0 the located point (kappa_0, r_0 interpolated with u, d_0 = (1.0 - u)*h),
//         node k >= 1 sample n_k = i + k (row index n_k mod N), d_k = h;
//         K_lim = min(K_cap, closed ? N : N - 1 - i)
//     march (serial): w_0 = v0, tt_0 = 0.0; w_0 == r_0: K* = 0.  Else for k = 0, 1, ..:
//         (a_acc, a_brk) = ax_max_at(cfg, w_k, kappa_k)
//         up = sqrt(smax(0.0, w_k*w_k + (2.0*a_acc)*d_k)), dn = sqrt(smax(0.0, w_k*w_k - (2.0*a_brk)*d_k))
//         w_{k+1} = smin(up, smax(dn, r_{k+1})), tt_{k+1} = tt_k + (2.0*d_k)/smax(1e-6, w_k + w_{k+1})
//         the first k + 1 with w_{k+1} == r_{k+1} is K*; none by K_lim: K* = -1; K_end = K* >= 0 ? K* : K_lim
//     merge: c0 = floor(n_K* / N), j* = n_K* - c0*N, t_ref = K* == 0 ? t0 : t[j*],
//         t_merge = tt_{K_end}, t_loss = tt_K* - (((double)c0*T + t_ref) - t0) (NaN when K* = -1)
//     ticks: tau_m = (double)m*dt.  M1 = #{m < M_cap : tau_m < tt_{K_end}} of them lie between the
//         nodes k, k + 1 with tt_k <= tau_m < tt_{k+1}, u_m = (tau_m - tt_k)/(tt_{k+1} - tt_k), the
//         columns interpolated between the node values, v between w_k and w_{k+1}, ax constant.
//         Merged rows go on at the row time t_ref + (tau_m - tt_K*) with §3l's wrap, bisection and
//         columns, c0 laps added to the count in s.
// raceline.rejoin_host states the same in NumPy, and the two agree bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_rejoin.h"

namespace rl {

// One workgroup per query, in the horizon kernel's steps with a march in the middle.  The locate
// is hzn_locate; its barrier also publishes the stamps of a row of N <= TRAJ_LDS_N samples.
// All lanes then stage kappa_k and r_k of the nodes k <= K_lim into LDS; lane 0 marches over
// them, writes w_k and tt_k beside them and hands K*, K_end, the counts and the merge time over
// through LDS; all lanes stride over the ticks (consecutive lanes, consecutive ticks) and over
// the nodes' w, tt for node_v, node_t.  No atomics: every output element has one writer.
// LDS: the stamps (32 776 B) and four node arrays (4 x 8 200 B).
__global__ __launch_bounds__(HZN_THREADS) void rl_rejoin_kernel(RjnParams rp) {
    __shared__ double s_t[TRAJ_LDS_N + 1];
    __shared__ double s_kap[RJN_MAX_NODES + 1];
    __shared__ double s_r[RJN_MAX_NODES + 1];
    __shared__ double s_w[RJN_MAX_NODES + 1];
    __shared__ double s_tt[RJN_MAX_NODES + 1];
    __shared__ uint64_t s_key[HZN_THREADS / 64];
    __shared__ uint32_t s_idx[HZN_THREADS / 64];
    __shared__ double s_tref;
    __shared__ int s_kstar, s_kend, s_m1, s_count;
    const HznParams& p = rp.hz;
    const TrajParams& q = p.src;
    const int k = blockIdx.x, tid = threadIdx.x, N = q.N;
    const int S = q.closed ? N : N - 1;
    const int r = p.row ? p.row[k] : 0, b = hzn_instance(q, r);
    if (b < 0 || b >= q.B || S < 1) {             // no row, or a row without a segment
        if (tid == 0) march_empty(rp, k);
        return;
    }
    const HznRow row = hzn_row(q, b);
    const double* tg = hzn_stamps(q, r);
    const bool lds = N <= TRAJ_LDS_N;
    if (lds)
        for (int i = tid; i <= N; i += HZN_THREADS) s_t[i] = tg[i];
    const double px = p.pose[2 * (size_t)k], py = p.pose[2 * (size_t)k + 1];

    const HznWin win = hzn_locate(p, k, tid, row.x, row.y, px, py, s_key, s_idx);
    if (win.key >= HZN_KEY_NAN || win.idx >= (uint32_t)S) {  // a NaN winner, or no candidate at all
        if (tid == 0) march_empty(rp, k);
        return;
    }
    auto stamp = [&](int i) { return lds ? s_t[i] : tg[i]; };
    const double h = hzn_step(q, b);
    const double T = q.T[r];
    // the located point, by every lane (the horizon kernel: lane 0 only): node 0 needs it in the tick phase
    const int i0 = (int)win.idx;
    const Foot f = hzn_foot(row.x, row.y, N, i0, px, py);
    const double t0 = hzn_t0(stamp, i0, f.u);
    const int room = q.closed ? N : N - 1 - i0;   // >= 1: i0 < S
    const int K_lim = rp.K_cap < room ? rp.K_cap : room;
    const March mr = march_from(row, s_kap, f, i0, N, h);
    const double d0 = mr.d0;
    march_stage(mr, tid, K_lim, s_kap, s_r);
    __syncthreads();
    if (tid == 0) {
        double w = rp.v0[k], tt = 0.0;
        int ks = -1, over = 0;
        s_w[0] = w;
        s_tt[0] = 0.0;
        if (w == s_r[0]) {
            ks = 0;
        } else {
            over += w > s_r[0];
            for (int kk = 0; kk < K_lim; ++kk) {
                const double d = kk == 0 ? d0 : h;
                const Reach s = march_step(rp.cfg, w, s_kap[kk], d);
                const double rn = s_r[kk + 1];
                const double wn = smin(s.up, smax(s.dn, rn));
                tt = march_time(tt, d, w, wn);
                s_w[kk + 1] = wn;
                s_tt[kk + 1] = tt;
                w = wn;
                if (wn == rn) {
                    ks = kk + 1;
                    break;
                }
                over += wn > rn;
            }
        }
        const int kend = ks >= 0 ? ks : K_lim;
        const double tte = s_tt[kend];
        const int nk = i0 + (ks >= 0 ? ks : 0), c0 = nk >= N ? 1 : 0;
        const double tref = ks == 0 ? t0 : stamp(nk - c0 * N);
        // M1: the first m with !(tau_m < tt_{K_end}); on a merged open row, the count: the first
        // m >= M1 whose row time is not < T
        const int m1 = tick_end(0, p.M_cap, [&](int m) { return (double)m * p.dt < tte; });
        int cnt = m1;
        if (ks >= 0) {
            if (!q.closed) cnt = tick_end(m1, p.M_cap, [&](int m) { return tref + ((double)m * p.dt - tte) < T; });
            else if (__builtin_isfinite(T) && T > 0.0) cnt = p.M_cap;
        }
        hzn_store_loc(p, k, f, i0, h, t0, cnt);
        rp.merge_node[k] = ks;
        rp.overspeed[k] = over;
        rp.scal[0][k] = tte;
        rp.scal[1][k] = ks >= 0 ? tte - (((double)c0 * T + tref) - t0) : __longlong_as_double(0x7ff8000000000000ll);
        s_tref = tref;
        s_kstar = ks;
        s_kend = kend;
        s_m1 = m1;
        s_count = cnt;
    }
    __syncthreads();
    const int kend = s_kend, m1 = s_m1, M = s_count;
    const int c0 = (s_kstar > 0 && i0 + s_kstar >= N) ? 1 : 0;
    const double tref = s_tref, tte = s_tt[kend];
    const size_t nrow = (size_t)k * ((size_t)rp.K_cap + 1);
    for (int kk = tid; kk <= kend; kk += HZN_THREADS) {
        rp.node_v[nrow + kk] = s_w[kk];
        rp.node_t[nrow + kk] = s_tt[kk];
    }
    const size_t orow = (size_t)k * (size_t)p.M_cap;
    for (int m = tid; m < M; m += HZN_THREADS) {
        const double tau = (double)m * p.dt;
        const size_t o = orow + m;
        if (m < m1) {
            march_columns(p, mr, s_w, s_tt, kend, tau, o);
        } else {
            const HznLap l = hzn_wrap(q.closed, T, tref + (tau - tte));
            hzn_columns(p, row, stamp, N, S, h, (double)c0 + l.c, l.w, o);
        }
    }
}

hipError_t launch_rejoin(const RjnParams& p, hipStream_t st) {
    hipLaunchKernelGGL(rl_rejoin_kernel, dim3((unsigned)p.hz.Q), dim3(HZN_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace rl
