// rl_rejoin.h — launch interface of the rejoin stage's kernel (rl_rejoin.hip): the
// horizon stage's query with the car's speed and limits: a reachable speed profile is marched
// from the located point until it meets the row's own, and the ticks follow it (rl_stages.cpp
// rl_plan_rejoin, rl_abi.cpp rl_rejoin).  Below it, the device functions of that kernel which
// the stop stage's kernel (rl_stop.hip) shares: the empty answer, ax_max_at and the
// march's step, the march nodes and their set-up, and a march tick's columns.  Not part of the
// public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rl_horizon.h"

namespace rl {

constexpr int RJN_MAX_NODES = 1024;     // RL_RJN_MAX_NODES: march nodes kept in LDS
constexpr int RJN_SCAL = 2;             // t_merge, t_loss (rl_rjn's order)

// the query's rl_cfg as ax_max_at reads it: the constant prefixes evaluated on the host, in the
// order VConst's are (rl_device.h), the rest copied
struct RjnCfg {
    double a_total2;    // a_total^2, a_total = use_total_ge_lat ? smax(a_total_max, a_lat_max) : a_total_max
    double kFd;         // 0.5*rho_air*Cd*A_front_m2
    double Fr;          // mass_kg*9.81*c_rr
    double mass, Pmax, acc_cap, brk_cap;
};

struct RjnParams {
    HznParams hz;              // the horizon stage's query and outputs, as launch_horizon takes them
    RjnCfg cfg;
    const double* v0;          // [Q]
    int32_t* merge_node;       // [Q]
    int32_t* overspeed;        // [Q]
    double* scal[RJN_SCAL];    // [Q] each
    double* node_v;            // [Q][K_cap + 1]
    double* node_t;            // [Q][K_cap + 1]
    int32_t K_cap;
};
// one workgroup per query; the conditions of launch_horizon, and 1 <= K_cap <= RJN_MAX_NODES
hipError_t launch_rejoin(const RjnParams& p, hipStream_t st);

// ------------------------------------------------------------------ shared device functions
// ax_max_at (ref:797-824) with the constant prefixes of RjnCfg, in the reference's operation
// order and its select forms of std::max / std::min
struct AxMax {
    double acc, brk;
};
__device__ __forceinline__ AxMax ax_max_at(const RjnCfg& c, double vi, double ki) {
    const double alat = vi * vi * fabs(ki);
    const double a_res = sqrt(smax(0.0, c.a_total2 - alat * alat));
    const double Fd = c.kFd * vi * vi;
    const double a_power = (c.Pmax > 0 && vi > 1e-6) ? (c.Pmax / (c.mass * vi) - (Fd + c.Fr) / c.mass) : 1e9;
    AxMax r;
    r.acc = smax(0.0, smin(smin(a_res, c.acc_cap), a_power));
    r.brk = smax(0.0, smin(a_res, c.brk_cap) + (Fd + c.Fr) / c.mass);
    return r;
}

// one step of the march from the speed w at a node of curvature kappa over the distance d: the
// fastest and the slowest speed at the next node; and that node's time, reached at wn
struct Reach {
    double up, dn;
};
__device__ __forceinline__ Reach march_step(const RjnCfg& c, double w, double kappa, double d) {
    const AxMax a = ax_max_at(c, w, kappa);
    return {sqrt(smax(0.0, w * w + (2.0 * a.acc) * d)), sqrt(smax(0.0, w * w - (2.0 * a.brk) * d))};
}
__device__ __forceinline__ double march_time(double tt, double d, double w, double wn) {
    return tt + (2.0 * d) / smax(1e-6, w + wn);
}

// the answer of a query without a row or without a winner, by the calling lane
__device__ __forceinline__ void march_empty(const RjnParams& rp, int k) {
    hzn_empty(rp.hz, k);
    rp.merge_node[k] = -1;
}

// position, heading, curvature and arc length of a march node
struct Node {
    double x, y, psi, kap, s;
};

// The march nodes of a located pose: node 0 the located point (segment i0 -> j0 at u), node
// k >= 1 sample i0 + k (row index mod N), d_0 = d0 and d_k = h; kap: the nodes' curvatures as
// march_stage left them in LDS.
struct March {
    HznRow row;
    const double* kap;
    double u, h, d0;
    int i0, j0, N;
};
// the march from the foot f on segment i0 (kap: where march_stage will put the curvatures)
__device__ __forceinline__ March march_from(const HznRow& row, const double* kap, const Foot& f, int i0, int N, double h) {
    return {row, kap, f.u, h, (1.0 - f.u) * h, i0, i0 + 1 < N ? i0 + 1 : 0, N};
}
__device__ __forceinline__ int march_sample(const March& m, int kk) {   // row index of node kk >= 1 (i0 + kk < 2N)
    const int n = m.i0 + kk;
    return n >= m.N ? n - m.N : n;
}
// all lanes: kappa_k and r_k of the nodes k <= K_lim into LDS (the caller's barrier publishes them)
__device__ __forceinline__ void march_stage(const March& m, int tid, int K_lim, double* s_kap, double* s_r) {
    for (int kk = tid; kk <= K_lim; kk += HZN_THREADS) {
        if (kk == 0) {
            const double ki = m.row.kap[m.i0], vi = m.row.v[m.i0];
            s_kap[0] = ki + m.u * (m.row.kap[m.j0] - ki);
            s_r[0] = vi + m.u * (m.row.v[m.j0] - vi);
        } else {
            const int n = march_sample(m, kk);
            s_kap[kk] = m.row.kap[n];
            s_r[kk] = m.row.v[n];
        }
    }
}
__device__ __forceinline__ Node march_node(const March& m, int kk) {
    Node n;
    if (kk == 0) {
        const double xi = m.row.x[m.i0], yi = m.row.y[m.i0], pi = m.row.psi[m.i0];
        double d = m.row.psi[m.j0] - pi;
        if (d > M_PI) d -= 2.0 * M_PI;
        else if (d < -M_PI) d += 2.0 * M_PI;
        n.x = xi + m.u * (m.row.x[m.j0] - xi);
        n.y = yi + m.u * (m.row.y[m.j0] - yi);
        n.psi = pi + m.u * d;
        n.s = ((double)m.i0 + m.u) * m.h;
    } else {
        const int j = march_sample(m, kk);
        n.x = m.row.x[j];
        n.y = m.row.y[j];
        n.psi = m.row.psi[j];
        n.s = (double)(m.i0 + kk) * m.h;
    }
    n.kap = m.kap[kk];
    return n;
}
// a tick's seven columns at the time tau on the march w, tt over the nodes 0 .. kend
// (tt_0 <= tau < tt_kend), written to element o of p.out: §3m's bisection and columns
__device__ __forceinline__ void march_columns(const HznParams& p, const March& m, const double* s_w, const double* s_tt,
                                              int kend, double tau, size_t o) {
    int a = 0, e = kend;                       // tt_a <= tau < tt_e
    while (e - a > 1) {
        const int mid = a + ((e - a) >> 1);
        if (s_tt[mid] <= tau) a = mid;
        else e = mid;
    }
    const double ta = s_tt[a], tb = s_tt[a + 1], wa = s_w[a], wb = s_w[a + 1];
    const double u = (tau - ta) / (tb - ta);
    const double d = a == 0 ? m.d0 : m.h;
    const Node A = march_node(m, a), B = march_node(m, a + 1);
    double dp = B.psi - A.psi;
    if (dp > M_PI) dp -= 2.0 * M_PI;
    else if (dp < -M_PI) dp += 2.0 * M_PI;
    p.out[0][o] = A.s + u * (B.s - A.s);
    p.out[1][o] = A.x + u * (B.x - A.x);
    p.out[2][o] = A.y + u * (B.y - A.y);
    p.out[3][o] = A.psi + u * dp;
    p.out[4][o] = A.kap + u * (B.kap - A.kap);
    p.out[5][o] = wa + u * (wb - wa);
    p.out[6][o] = d > 0.0 ? (wb * wb - wa * wa) / (2.0 * d) : 0.0;
}

}  // namespace rl
