// rl_recover.h — launch interface of the recover stage's kernel (rl_recover.hip): the
// rejoin stage's query with a merge length and the car's direction, answered with a lateral
// offset profile from the car's offset to zero inside the bounds stage's free width, the
// geometry of that offset path, the retime stage's speed pass on it and the ticks along it
// (rl_stages.cpp rl_plan_recover, rl_abi.cpp rl_recover).  Below it, the phases of that kernel as
// device functions, which the fan stage's kernels (rl_recover_fan.hip) share: the
// locate, the offsets and their clamp, the points, d', kappa' and psi, the ceiling, the pass, the
// per-query values and a tick's columns.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rl_math.h"
#include "rl_retime.h"

namespace rl {

constexpr int RCV_MAX_NODES = 512;      // RL_RCV_MAX_NODES: the nodes' arrays kept in LDS
constexpr int RCV_SCAL = 2;             // lo0, hi0: the doubles beyond the retime stage's
constexpr int RCV_INTS = 3;             // clamped, offtrack, merge_node: the ints beyond the retime stage's
constexpr int RCV_NODES = 2;            // node_o, node_k: the node arrays beyond the retime stage's

struct RcvParams {
    // the retime stage's query and outputs as launch_retime takes them, with the same meaning
    RtmParams rt;
    const double* merge_len;       // [Q]
    const double* dir;             // [Q][2]; nullptr: g0 = 0.0
    // the bounds stage's rows, row r the trajectory stage's row r
    const double *lo, *hi, *nx, *ny;   // [R][N]
    double* offset;                // [Q][M_cap]
    double* scal[RCV_SCAL];        // [Q] each
    int32_t* clamped;              // [Q]
    int32_t* offtrack;             // [Q]
    int32_t* merge_node;           // [Q]
    double* node_o;                // [Q][K_cap + 1]
    double* node_k;                // [Q][K_cap + 1]
};
// one workgroup per query; the conditions of launch_rejoin, and K_cap <= RCV_MAX_NODES
hipError_t launch_recover(const RcvParams& p, hipStream_t st);

// ------------------------------------------------------------------ shared device functions
// the LDS of one query: eleven node arrays and the waves' meeting places
struct RcvShared {
    double kap[RCV_MAX_NODES + 1];    // kappa_k, then c_k
    double r[RCV_MAX_NODES + 1];
    double o[RCV_MAX_NODES + 1];
    double px[RCV_MAX_NODES + 1];
    double py[RCV_MAX_NODES + 1];
    double d[RCV_MAX_NODES + 1];
    double kp[RCV_MAX_NODES + 1];     // kappa'_k
    double psi[RCV_MAX_NODES + 1];
    double b[RCV_MAX_NODES + 1];
    double w[RCV_MAX_NODES + 1];
    double tt[RCV_MAX_NODES + 1];
    uint64_t key[HZN_THREADS / 64];
    uint32_t idx[HZN_THREADS / 64];
    int cl[HZN_THREADS / 64];
    int mg[HZN_THREADS / 64];
    int m1;
};

// the located query, the same in every lane: its row and stamps, the bounds stage's rows of that
// row, the foot, the march, the car's offset e, the merge length D and g0*D, and K
struct RcvGeo {
    HznRow row;
    const double* tg;
    const double *blo, *bhi, *bnx, *bny;
    Foot f;
    March mr;
    double h, e, D, gD;
    int r, i0, K;
};

// the nodes' arrays a curvature, a heading or a tick reads
struct RcvNodes {
    const double *o, *px, *py, *d, *kap;
    int K;
};

// whether node kk is on the line: o == 0.0 at kk - 1, kk and kk + 1 within [0, K]
__device__ __forceinline__ bool rcv_on_line(const RcvNodes& n, int kk) {
    return n.o[kk] == 0.0 && (kk == 0 || n.o[kk - 1] == 0.0) && (kk == n.K || n.o[kk + 1] == 0.0);
}

// kappa' of an interior node kk (1 <= kk <= K - 1): the row's on the line, else Menger's
__device__ __forceinline__ double rcv_kappa_inner(const RcvNodes& n, int kk) {
    if (rcv_on_line(n, kk)) return n.kap[kk];
    const double ax = n.px[kk] - n.px[kk - 1], ay = n.py[kk] - n.py[kk - 1];
    const double bx = n.px[kk + 1] - n.px[kk], by = n.py[kk + 1] - n.py[kk];
    const double cx = n.px[kk + 1] - n.px[kk - 1], cy = n.py[kk + 1] - n.py[kk - 1];
    const double den = (n.d[kk - 1] * n.d[kk]) * sqrt(cx * cx + cy * cy);
    return den > 0.0 ? (2.0 * (ax * by - ay * bx)) / den : 0.0;
}

// kappa' of any node kk: an end node off the line takes its neighbour's when there is an
// interior node, else the row's
__device__ __forceinline__ double rcv_kappa(const RcvNodes& n, int kk) {
    if (kk > 0 && kk < n.K) return rcv_kappa_inner(n, kk);
    if (n.K < 2 || rcv_on_line(n, kk)) return n.kap[kk];
    return rcv_kappa_inner(n, kk == 0 ? 1 : n.K - 1);
}

// the heading of a node kk off the line: the direction of the chord across it
__device__ __forceinline__ double rcv_psi(const RcvNodes& n, int kk) {
    const int a = kk == 0 ? 0 : kk - 1, b = kk == n.K ? n.K : kk + 1;
    return atan2_cr(n.py[b] - n.py[a], n.px[b] - n.px[a]);
}

// The locate and the nodes of query kq (pose, row, hint, dir at kq; D = merge_len[kd]) by the
// whole workgroup: hzn_locate, the foot, K, the march, e, g0 and the row's kappa_k, r_k staged
// into LDS (the next barrier publishes them).  false: a query without a row, a winner or a node
// ahead, whose empty answer lane 0 has written at ko.
__device__ __forceinline__ bool rcv_begin(const RcvParams& cp, int kq, int kd, int ko, int tid, RcvShared& sh, RcvGeo& g) {
    const RjnParams& rp = cp.rt.rj;
    const HznParams& p = rp.hz;
    const TrajParams& q = p.src;
    const int N = q.N;
    const int S = q.closed ? N : N - 1;
    const int r = p.row ? p.row[kq] : 0, b = hzn_instance(q, r);
    if (b < 0 || b >= q.B || S < 1) {             // no row, or a row without a segment
        if (tid == 0) march_empty(rp, ko);
        return false;
    }
    g.r = r;
    g.row = hzn_row(q, b);
    g.tg = hzn_stamps(q, r);
    const double px = p.pose[2 * (size_t)kq], py = p.pose[2 * (size_t)kq + 1];

    const HznWin win = hzn_locate(p, kq, tid, g.row.x, g.row.y, px, py, sh.key, sh.idx);
    if (win.key >= HZN_KEY_NAN || win.idx >= (uint32_t)S) {  // a NaN winner, or no candidate at all
        if (tid == 0) march_empty(rp, ko);
        return false;
    }
    g.h = hzn_step(q, b);
    // the located point, by every lane: every pass needs it
    g.i0 = (int)win.idx;
    g.f = hzn_foot(g.row.x, g.row.y, N, g.i0, px, py);
    const int room = q.closed ? N : N - 1 - g.i0;   // >= 1: i0 < S
    int K = rp.K_cap < room ? rp.K_cap : room;
    if (K > RCV_MAX_NODES) K = RCV_MAX_NODES;     // (the entry points refuse such a K_cap: the nodes fit the LDS arrays)
    if (K < 1) {                                   // no node ahead (the same for every lane)
        if (tid == 0) march_empty(rp, ko);
        return false;
    }
    g.K = K;
    g.mr = march_from(g.row, sh.kap, g.f, g.i0, N, g.h);
    // the bounds stage's rows of this query's row
    const size_t boff = (size_t)r * (size_t)N;
    g.blo = cp.lo + boff;
    g.bhi = cp.hi + boff;
    g.bnx = cp.nx + boff;
    g.bny = cp.ny + boff;
    // the car's offset, slope and merge length, by every lane
    const Foot& f = g.f;
    const double root = sqrt(f.D);
    g.e = (f.dx * f.wy - f.dy * f.wx) < 0.0 ? -root : root;   // hzn_store_loc's e
    g.D = cp.merge_len[kd];
    double g0 = 0.0;
    if (cp.dir) {
        const double hx = cp.dir[2 * (size_t)kq], hy = cp.dir[2 * (size_t)kq + 1];
        const double den = f.dx * hx + f.dy * hy, num = f.dx * hy - f.dy * hx;
        g0 = den > 0.0 ? smin(1.0, smax(-1.0, num / den)) : (num < 0.0 ? -1.0 : (num > 0.0 ? 1.0 : 0.0));
    }
    g.gD = g0 * g.D;
    march_stage(g.mr, tid, K, sh.kap, sh.r);
    return true;
}

// offsets and clamp, one node per lane, strided; the waves count the clamped nodes and find the
// merge node with a butterfly each and leave both in LDS
__device__ __forceinline__ void rcv_offsets(const RcvGeo& g, int tid, RcvShared& sh) {
    int ncl = 0, mg = 0x7fffffff;
    for (int kk = tid; kk <= g.K; kk += HZN_THREADS) {
        if (kk == 0) {
            sh.o[0] = g.e;
            continue;
        }
        const double a = g.mr.d0 + (double)(kk - 1) * g.h;
        const double z = smin(1.0, a / g.D);
        const double z3 = (z * z) * z;
        const double qz = 1.0 + z3 * (-10.0 + z * (15.0 - 6.0 * z));
        const double pz = z + z3 * (-6.0 + z * (8.0 - 3.0 * z));
        const double raw = g.e * qz + g.gD * pz;
        const int n = march_sample(g.mr, kk);
        const double o = smin(g.bhi[n], smax(g.blo[n], raw));
        sh.o[kk] = o;
        ncl += o != raw;
        if (z >= 1.0 && kk < mg) mg = kk;
    }
    for (int off = 32; off; off >>= 1) {
        ncl += __shfl_xor(ncl, off, 64);
        const int om = __shfl_xor(mg, off, 64);
        mg = om < mg ? om : mg;
    }
    if ((tid & 63) == 0) {
        sh.cl[tid >> 6] = ncl;
        sh.mg[tid >> 6] = mg;
    }
}

// points
__device__ __forceinline__ void rcv_points(const RcvGeo& g, int tid, RcvShared& sh) {
    const Foot& f = g.f;
    for (int kk = tid; kk <= g.K; kk += HZN_THREADS) {
        if (kk == 0) {
            const Node n0 = march_node(g.mr, 0);
            sh.px[0] = n0.x + (f.wx - f.u * f.dx);
            sh.py[0] = n0.y + (f.wy - f.u * f.dy);
        } else {
            const int n = march_sample(g.mr, kk);
            const double o = sh.o[kk];
            sh.px[kk] = g.row.x[n] + o * g.bnx[n];
            sh.py[kk] = g.row.y[n] + o * g.bny[n];
        }
    }
}

// d': the segments' lengths
__device__ __forceinline__ void rcv_lengths(const RcvGeo& g, int tid, RcvShared& sh) {
    for (int kk = tid; kk < g.K; kk += HZN_THREADS) {
        if (sh.o[kk] == 0.0 && sh.o[kk + 1] == 0.0) {
            sh.d[kk] = kk == 0 ? g.mr.d0 : g.h;
        } else {
            const double qx = sh.px[kk + 1] - sh.px[kk], qy = sh.py[kk + 1] - sh.py[kk];
            sh.d[kk] = sqrt(qx * qx + qy * qy);
        }
    }
}

// kappa' and psi: the nodes' curvatures and headings
__device__ __forceinline__ void rcv_curvatures(const RcvGeo& g, int tid, RcvShared& sh) {
    const RcvNodes nd = {sh.o, sh.px, sh.py, sh.d, sh.kap, g.K};
    for (int kk = tid; kk <= g.K; kk += HZN_THREADS) {
        sh.kp[kk] = rcv_kappa(nd, kk);
        sh.psi[kk] = rcv_on_line(nd, kk) ? march_node(g.mr, kk).psi : rcv_psi(nd, kk);
    }
}

// the ceiling, over the row's curvatures: nothing reads them after rcv_curvatures
__device__ __forceinline__ void rcv_ceiling(const RcvParams& cp, const RcvGeo& g, int tid, RcvShared& sh) {
    for (int kk = tid; kk <= g.K; kk += HZN_THREADS) sh.kap[kk] = retime_ceiling(cp.rt, sh.kp[kk], sh.r[kk]);
}

// the pass, by the calling lane: the retime stage's envelope and march over LDS with v0 of query
// kq, the location and the retime stage's per-query values stored at ko; the tick count into LDS
__device__ __forceinline__ void rcv_pass(const RcvParams& cp, const RcvGeo& g, int kq, int ko, RcvShared& sh) {
    const RtmParams& tp = cp.rt;
    const RjnParams& rp = tp.rj;
    const HznParams& p = rp.hz;
    const TrajParams& q = p.src;
    const double* s_c = sh.kap;
    const double* tg = g.tg;
    const int N = q.N, K = g.K, i0 = g.i0;
    const double v0 = rp.v0[kq];
    const RtmPass ps = retime_pass(rp.cfg, v0, K, sh.kp, sh.r, s_c, sh.b, sh.w, sh.tt, [&](int kk) { return sh.d[kk]; });
    const double tte = ps.tt;
    const int m1 = tick_end(0, p.M_cap, [&](int m) { return (double)m * p.dt < tte; });
    const double t0 = hzn_t0([&](int i) { return tg[i]; }, i0, g.f.u);
    const int nk = i0 + K, c0 = nk >= N ? 1 : 0;   // nk < 2N
    hzn_store_loc(p, ko, g.f, i0, g.h, t0, m1);
    rp.merge_node[ko] = K;                         // end_node
    rp.overspeed[ko] = ps.over;
    rp.scal[0][ko] = tte;
    rp.scal[1][ko] = tte - (((double)c0 * q.T[g.r] + tg[nk - c0 * N]) - t0);
    tp.feasible[ko] = v0 <= sh.b[0] ? 1 : 0;
    tp.bind_node[ko] = ps.bn;
    tp.v_excess[ko] = ps.ve;
    sh.m1 = m1;
}

// the offsets' per-query values at ko, by the calling lane
__device__ __forceinline__ void rcv_values(const RcvParams& cp, const RcvGeo& g, int ko, const RcvShared& sh) {
    int cl = 0, m = 0x7fffffff;
    for (int w = 0; w < HZN_THREADS / 64; ++w) {
        cl += sh.cl[w];
        m = sh.mg[w] < m ? sh.mg[w] : m;
    }
    const int i0 = g.i0, j0 = g.mr.j0;
    const double lo0 = smax(g.blo[i0], g.blo[j0]), hi0 = smin(g.bhi[i0], g.bhi[j0]);
    cp.clamped[ko] = cl;
    cp.merge_node[ko] = m == 0x7fffffff ? -1 : m;
    cp.offtrack[ko] = !(lo0 <= g.e && g.e <= hi0) ? 1 : 0;
    cp.scal[0][ko] = lo0;
    cp.scal[1][ko] = hi0;
}

// One query up to and including the serial passes, by the whole workgroup: rcv_begin, then the
// five parallel passes with a barrier after each, then lane 0 runs the pass and lane 64 the
// offsets' per-query values; the last barrier publishes the march and the tick count.  false: an
// empty query (answered).
__device__ __forceinline__ bool rcv_solve(const RcvParams& cp, int kq, int kd, int ko, int tid, RcvShared& sh, RcvGeo& g) {
    if (!rcv_begin(cp, kq, kd, ko, tid, sh, g)) return false;
    rcv_offsets(g, tid, sh);
    __syncthreads();
    rcv_points(g, tid, sh);
    __syncthreads();
    rcv_lengths(g, tid, sh);
    __syncthreads();
    rcv_curvatures(g, tid, sh);
    __syncthreads();
    rcv_ceiling(cp, g, tid, sh);
    __syncthreads();
    if (tid == 0) rcv_pass(cp, g, kq, ko, sh);
    else if (tid == 64) rcv_values(cp, g, ko, sh);     // off lane 0
    __syncthreads();
    return true;
}

// the nodes a tick lies between, and where the car was located: the arrays over 0 .. K
struct RcvTicks {
    const double *o, *px, *py, *d, *kp, *psi, *w, *tt;
    double u, h;
    int i0, K;
};

// a tick's eight columns at the time tau (tt_0 <= tau < tt_K), written to element o of the
// columns: march_columns' bisection, then the columns between the nodes' P, psi, kappa', w, s, o
__device__ __forceinline__ void rcv_tick(const RcvParams& cp, const RcvTicks& n, double tau, size_t o) {
    const HznParams& p = cp.rt.rj.hz;
    int a = 0, en = n.K;                           // tt_a <= tau < tt_en
    while (en - a > 1) {
        const int mid = a + ((en - a) >> 1);
        if (n.tt[mid] <= tau) a = mid;
        else en = mid;
    }
    const double ta = n.tt[a], tb = n.tt[a + 1], wa = n.w[a], wb = n.w[a + 1];
    const double u = (tau - ta) / (tb - ta);
    const double d = n.d[a];
    const double sa = a == 0 ? ((double)n.i0 + n.u) * n.h : (double)(n.i0 + a) * n.h, sb = (double)(n.i0 + a + 1) * n.h;
    const double pa = n.psi[a];
    double dp = n.psi[a + 1] - pa;
    if (dp > M_PI) dp -= 2.0 * M_PI;
    else if (dp < -M_PI) dp += 2.0 * M_PI;
    p.out[0][o] = sa + u * (sb - sa);
    p.out[1][o] = n.px[a] + u * (n.px[a + 1] - n.px[a]);
    p.out[2][o] = n.py[a] + u * (n.py[a + 1] - n.py[a]);
    p.out[3][o] = pa + u * dp;
    p.out[4][o] = n.kp[a] + u * (n.kp[a + 1] - n.kp[a]);
    p.out[5][o] = wa + u * (wb - wa);
    p.out[6][o] = d > 0.0 ? (wb * wb - wa * wa) / (2.0 * d) : 0.0;
    cp.offset[o] = n.o[a] + u * (n.o[a + 1] - n.o[a]);
}

}  // namespace rl
