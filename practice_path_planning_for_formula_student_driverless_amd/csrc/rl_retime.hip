// rl_retime.hip — the retime stage's kernel: "I am at (px, py) doing v0 and my limits
// have changed: what speed profile do I drive over the nodes ahead, where do today's limits first
// fall below the plan, and what does that cost?"  The rejoin stage's query (rl_rejoin.hip, §3m)
// answered with the reference's forward/backward speed pass under the query's cfg.  Per query, in
// fp64 without contraction:
//     locate, nodes: the rejoin stage's: seg = i, u, e, dist2, t0, s0; kappa_k, r_k, d_k, n_k = i + k,
//         K = K_lim
//     ceiling (per node): c_k = smin(smin(v_cap, sqrt(a_lat_max / smax(fabs(kappa_k), kappa_eps))), r_k)
//     envelope (serial, backward): b_K = c_K; for k = K - 1 .. 0:
//         (., a_brk) = ax_max_at(cfg, b_{k+1}, kappa_{k+1}),
//         b_k = smin(c_k, sqrt(smax(0.0, b_{k+1}*b_{k+1} + (2.0*a_brk)*d_k)));  feasible = v0 <= b_0
//     march (serial, forward, always to K): w_0 = v0, tt_0 = 0.0; for k = 0 .. K - 1:
//         (up, dn) = march_step(cfg, w_k, kappa_k, d_k)
//         w_{k+1} = smin(up, w_k <= b_k ? b_{k+1} : smax(dn, b_{k+1})), tt_{k+1} = march_time(tt_k, d_k, w_k, w_{k+1})
//     per query: overspeed = #{k <= K : w_k > b_k}, v_excess the largest w_k - b_k or 0.0; bind_node
//         the first k with b_k < r_k (none: -1); t_end = tt_K;
//         t_loss = tt_K - (((double)c0*T + t[j_K]) - t0), c0 = floor(n_K / N), j_K = n_K - c0*N
//     ticks: tau_m = (double)m*dt; count = #{m < M_cap : tau_m < tt_K}, all of them on the march,
//         with the rejoin stage's node bisection and march-tick columns
// raceline.retime_host states the same in NumPy, and the two agree bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_retime.h"

namespace rl {

// One workgroup per query, in the stop kernel's steps with a parallel pass before the serial
// ones.  The locate is hzn_locate.  All lanes stage kappa_k and r_k of the nodes k <= K into LDS,
// then compute the ceiling c_k, one node per lane, strided: that part of the reference's pass has
// no dependence between nodes.  Lane 0 sweeps the envelope backward and marches forward over
// LDS, writes b_k, w_k and tt_k beside them and hands the tick count over through LDS; all lanes
// stride over the ticks (consecutive lanes, consecutive ticks) and over the nodes' w, tt, b, c
// for the node arrays.  No atomics: every output element has one writer.  Of the stamps only
// the located segment's two (t0) and the last node's and T (t_loss) are needed; they come from
// global memory.  LDS: six node arrays (6 x 8 200 B).
__global__ __launch_bounds__(HZN_THREADS) void rl_retime_kernel(RtmParams tp) {
    __shared__ double s_kap[RJN_MAX_NODES + 1];
    __shared__ double s_r[RJN_MAX_NODES + 1];
    __shared__ double s_c[RJN_MAX_NODES + 1];
    __shared__ double s_b[RJN_MAX_NODES + 1];
    __shared__ double s_w[RJN_MAX_NODES + 1];
    __shared__ double s_tt[RJN_MAX_NODES + 1];
    __shared__ uint64_t s_key[HZN_THREADS / 64];
    __shared__ uint32_t s_idx[HZN_THREADS / 64];
    __shared__ int s_m1;
    const RjnParams& rp = tp.rj;
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
    const double px = p.pose[2 * (size_t)k], py = p.pose[2 * (size_t)k + 1];

    const HznWin win = hzn_locate(p, k, tid, row.x, row.y, px, py, s_key, s_idx);
    if (win.key >= HZN_KEY_NAN || win.idx >= (uint32_t)S) {  // a NaN winner, or no candidate at all
        if (tid == 0) march_empty(rp, k);
        return;
    }
    const double h = hzn_step(q, b);
    // the located point, by every lane: node 0 needs it in the tick phase
    const int i0 = (int)win.idx;
    const Foot f = hzn_foot(row.x, row.y, N, i0, px, py);
    const int room = q.closed ? N : N - 1 - i0;   // >= 1: i0 < S
    int K = rp.K_cap < room ? rp.K_cap : room;
    if (K > RJN_MAX_NODES) K = RJN_MAX_NODES;     // (the entry points refuse such a K_cap: the nodes fit the LDS arrays)
    if (K < 1) {                                   // no node ahead (the same for every lane)
        if (tid == 0) march_empty(rp, k);
        return;
    }
    const March mr = march_from(row, s_kap, f, i0, N, h);
    const double d0 = mr.d0;
    march_stage(mr, tid, K, s_kap, s_r);
    __syncthreads();
    for (int kk = tid; kk <= K; kk += HZN_THREADS) s_c[kk] = retime_ceiling(tp, s_kap[kk], s_r[kk]);
    __syncthreads();
    if (tid == 0) {
        const double v0 = rp.v0[k];
        const RtmPass ps = retime_pass(rp.cfg, v0, K, s_kap, s_r, s_c, s_b, s_w, s_tt, [&](int kk) { return kk == 0 ? d0 : h; });
        const double tte = ps.tt;
        const int m1 = tick_end(0, p.M_cap, [&](int m) { return (double)m * p.dt < tte; });
        const double t0 = hzn_t0([&](int i) { return tg[i]; }, i0, f.u);
        const int nk = i0 + K, c0 = nk >= N ? 1 : 0;   // nk < 2N
        hzn_store_loc(p, k, f, i0, h, t0, m1);
        rp.merge_node[k] = K;
        rp.overspeed[k] = ps.over;
        rp.scal[0][k] = tte;
        rp.scal[1][k] = tte - (((double)c0 * q.T[r] + tg[nk - c0 * N]) - t0);
        tp.feasible[k] = v0 <= s_b[0] ? 1 : 0;
        tp.bind_node[k] = ps.bn;
        tp.v_excess[k] = ps.ve;
        s_m1 = m1;
    }
    __syncthreads();
    const int M = s_m1;
    const size_t nrow = (size_t)k * ((size_t)rp.K_cap + 1);
    for (int kk = tid; kk <= K; kk += HZN_THREADS) {
        rp.node_v[nrow + kk] = s_w[kk];
        rp.node_t[nrow + kk] = s_tt[kk];
        tp.node_b[nrow + kk] = s_b[kk];
        tp.node_c[nrow + kk] = s_c[kk];
    }
    const size_t orow = (size_t)k * (size_t)p.M_cap;
    for (int m = tid; m < M; m += HZN_THREADS) march_columns(p, mr, s_w, s_tt, K, (double)m * p.dt, orow + m);
}

hipError_t launch_retime(const RtmParams& p, hipStream_t st) {
    hipLaunchKernelGGL(rl_retime_kernel, dim3((unsigned)p.rj.hz.Q), dim3(HZN_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace rl
