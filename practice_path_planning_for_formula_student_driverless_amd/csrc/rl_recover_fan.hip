// rl_recover_fan.hip — the fan stage's kernels: "I am off the line: which of these C
// merge lengths takes me back best?"  The recover stage (rl_recover.hip, §3q) C times per pose,
// then an exact order.  Per query q and candidate c, in fp64 without contraction:
//     candidate: the recover stage's answer for query q with D = merge_len[q][c], word for word
//     class: g = !feasible ? 3 : (merge_node < 0 ? 2 : (clamped != 0 ? 1 : 0))
//     order: ascending in (g, isnan(t_end), t_end, c), plain < on doubles; best = the first
//     results: the winner's, every field of the recover stage's; the table: every candidate's
//         class, feasible, clamped, merge_node, overspeed, bind_node, t_end, t_loss, v_excess
//     an empty query (the recover stage's end_node = -1): seg, count = 0, end_node = -1, best = -1
// raceline.recover_fan_host states the same in NumPy.  Two kernels on one stream, built from the
// recover kernel's phases (rl_recover.h), so that the C serial passes of a pose run on C CUs at
// once instead of one after the other on one lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_recover_fan.h"

namespace rl {

// The candidate kernel: one workgroup per candidate k = q*C + c, the recover kernel up to and
// including its serial passes (rcv_solve) on pose, v0, row, hint and dir of query q with
// D = merge_len[k].  The per-query values go to element k of the scratch block; so do the ten
// node arrays the select kernel needs for the winner's ticks and node arrays.  No ticks.
__global__ __launch_bounds__(HZN_THREADS) void rl_fan_candidate_kernel(FanParams fp) {
    __shared__ RcvShared sh;
    const RcvParams& cp = fp.cand;
    const RtmParams& tp = cp.rt;
    const RjnParams& rp = tp.rj;
    const int k = blockIdx.x, tid = threadIdx.x;
    RcvGeo g;
    if (!rcv_solve(cp, k / fp.C, k, k, tid, sh, g)) return;
    const double* s_c = sh.kap;
    const size_t nrow = (size_t)k * ((size_t)rp.K_cap + 1);
    for (int kk = tid; kk <= g.K; kk += HZN_THREADS) {
        rp.node_v[nrow + kk] = sh.w[kk];
        rp.node_t[nrow + kk] = sh.tt[kk];
        tp.node_b[nrow + kk] = sh.b[kk];
        tp.node_c[nrow + kk] = s_c[kk];
        cp.node_o[nrow + kk] = sh.o[kk];
        cp.node_k[nrow + kk] = sh.kp[kk];
        fp.xnode[0][nrow + kk] = sh.px[kk];
        fp.xnode[1][nrow + kk] = sh.py[kk];
        fp.xnode[2][nrow + kk] = kk < g.K ? sh.d[kk] : 0.0;   // (d' has K entries)
        fp.xnode[3][nrow + kk] = sh.psi[kk];
    }
}

// whether candidate (ga, ta) comes before (gb, tb) in (class, isnan(t_end), t_end); the index
// decides among equals: the caller scans it upward and keeps the first
__device__ __forceinline__ bool fan_before(int ga, double ta, int gb, double tb) {
    if (ga != gb) return ga < gb;
    const bool na = ta != ta, nb = tb != tb;
    if (na != nb) return nb;
    return ta < tb;
}

// The select kernel: one workgroup per query.  Lane c < C classifies candidate c from the scratch
// block and writes its table row; every lane then scans the C classes and times in LDS for the
// winner.  All lanes bring the winner's node arrays from scratch into LDS and out to the results;
// lane 0 copies its per-query values; all lanes stride over its ticks (rcv_tick).  No atomics:
// every output element has one writer.  LDS: eight node arrays (8 x 4 104 B).
__global__ __launch_bounds__(HZN_THREADS) void rl_fan_select_kernel(FanParams fp) {
    __shared__ double s_o[RCV_MAX_NODES + 1];
    __shared__ double s_px[RCV_MAX_NODES + 1];
    __shared__ double s_py[RCV_MAX_NODES + 1];
    __shared__ double s_d[RCV_MAX_NODES + 1];
    __shared__ double s_kp[RCV_MAX_NODES + 1];
    __shared__ double s_psi[RCV_MAX_NODES + 1];
    __shared__ double s_w[RCV_MAX_NODES + 1];
    __shared__ double s_tt[RCV_MAX_NODES + 1];
    __shared__ double s_t[FAN_MAX_CAND];
    __shared__ int s_g[FAN_MAX_CAND];
    const RcvParams &cp = fp.cand, &wp = fp.win;
    const RtmParams &ct = cp.rt, &wt = wp.rt;
    const RjnParams &cr = ct.rj, &wr = wt.rj;
    const HznParams &ch = cr.hz, &wh = wr.hz;
    const int q = blockIdx.x, tid = threadIdx.x, C = fp.C;
    const size_t k0 = (size_t)q * (size_t)C;
    // every candidate of a query shares the locate: all are empty or none is
    if (cr.merge_node[k0] < 0) {
        if (tid == 0) {
            wh.seg[q] = ch.seg[k0];
            wh.count[q] = 0;
            wr.merge_node[q] = -1;
            fp.best[q] = -1;
        }
        return;
    }
    if (tid < C) {
        const size_t k = k0 + tid;
        const int fe = ct.feasible[k], cl = cp.clamped[k], mn = cp.merge_node[k];
        const double te = cr.scal[0][k];
        const int g = !fe ? 3 : (mn < 0 ? 2 : (cl != 0 ? 1 : 0));
        s_g[tid] = g;
        s_t[tid] = te;
        fp.tab_i[0][k] = g;
        fp.tab_i[1][k] = fe;
        fp.tab_i[2][k] = cl;
        fp.tab_i[3][k] = mn;
        fp.tab_i[4][k] = cr.overspeed[k];
        fp.tab_i[5][k] = ct.bind_node[k];
        fp.tab_d[0][k] = te;
        fp.tab_d[1][k] = cr.scal[1][k];
        fp.tab_d[2][k] = ct.v_excess[k];
    }
    __syncthreads();
    int best = 0;                                      // the same in every lane
    for (int c = 1; c < C; ++c)
        if (fan_before(s_g[c], s_t[c], s_g[best], s_t[best])) best = c;
    const size_t kb = k0 + best;
    const int K = cr.merge_node[kb], M = ch.count[kb], i0 = ch.seg[kb];   // end_node, count, seg
    const double u = ch.loc[0][kb];
    const size_t crow = kb * ((size_t)cr.K_cap + 1), nrow = (size_t)q * ((size_t)wr.K_cap + 1);
    for (int kk = tid; kk <= K; kk += HZN_THREADS) {
        const double w = cr.node_v[crow + kk], tt = cr.node_t[crow + kk], o = cp.node_o[crow + kk], kp = cp.node_k[crow + kk];
        s_w[kk] = w;
        s_tt[kk] = tt;
        s_o[kk] = o;
        s_kp[kk] = kp;
        s_px[kk] = fp.xnode[0][crow + kk];
        s_py[kk] = fp.xnode[1][crow + kk];
        s_d[kk] = fp.xnode[2][crow + kk];
        s_psi[kk] = fp.xnode[3][crow + kk];
        wr.node_v[nrow + kk] = w;
        wr.node_t[nrow + kk] = tt;
        wt.node_b[nrow + kk] = ct.node_b[crow + kk];
        wt.node_c[nrow + kk] = ct.node_c[crow + kk];
        wp.node_o[nrow + kk] = o;
        wp.node_k[nrow + kk] = kp;
    }
    if (tid == 0) {
        fp.best[q] = best;
        wh.seg[q] = i0;
        wh.count[q] = M;
        for (int c = 0; c < HZN_LOC; ++c) wh.loc[c][q] = ch.loc[c][kb];
        wr.merge_node[q] = K;                          // end_node
        wr.overspeed[q] = cr.overspeed[kb];
        for (int c = 0; c < RJN_SCAL; ++c) wr.scal[c][q] = cr.scal[c][kb];
        wt.feasible[q] = ct.feasible[kb];
        wt.bind_node[q] = ct.bind_node[kb];
        wt.v_excess[q] = ct.v_excess[kb];
        wp.clamped[q] = cp.clamped[kb];
        wp.offtrack[q] = cp.offtrack[kb];
        wp.merge_node[q] = cp.merge_node[kb];
        for (int c = 0; c < RCV_SCAL; ++c) wp.scal[c][q] = cp.scal[c][kb];
    }
    __syncthreads();
    // the row's step, as the candidate kernel took it (a located query has a row)
    const TrajParams& src = wh.src;
    const double h = hzn_step(src, hzn_instance(src, wh.row ? wh.row[q] : 0));
    const RcvTicks nt = {s_o, s_px, s_py, s_d, s_kp, s_psi, s_w, s_tt, u, h, i0, K};
    const size_t orow = (size_t)q * (size_t)wh.M_cap;
    for (int m = tid; m < M; m += HZN_THREADS) rcv_tick(wp, nt, (double)m * wh.dt, orow + m);
}

hipError_t launch_recover_fan(const FanParams& p, hipStream_t st) {
    const unsigned Q = (unsigned)p.win.rt.rj.hz.Q;
    hipLaunchKernelGGL(rl_fan_candidate_kernel, dim3(Q * (unsigned)p.C), dim3(HZN_THREADS), 0, st, p);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(rl_fan_select_kernel, dim3(Q), dim3(HZN_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace rl
