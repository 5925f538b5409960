// rl_recover.hip — the recover stage's kernel: "I am at (px, py), e off the line and
// heading (hx, hy), doing v0: which path takes me back to the line within D metres without leaving
// the track, and how fast may I drive it?"  The rejoin stage's query (rl_rejoin.hip, §3m) with a
// merge length and a direction, answered on the bounds stage's rows (rl_bounds.hip, §3o) with the
// retime stage's speed pass (rl_retime.hip, §3p).  Per query, in fp64 without contraction:
//     locate, nodes: the rejoin stage's: seg = i, u, e, dist2, t0, s0; kappa_k, r_k, d_k, n_k = i + k,
//         K = K_lim
//     slope: den = dx*hx + dy*hy, num = dx*hy - dy*hx,
//         g0 = den > 0 ? smin(1.0, smax(-1.0, num/den)) : (num < 0 ? -1.0 : (num > 0 ? 1.0 : 0.0)); no dir: 0.0
//     offsets (per node): a_0 = 0.0, a_k = d_0 + (double)(k-1)*h, z = smin(1.0, a_k/D), z3 = (z*z)*z,
//         qz = 1.0 + z3*(-10.0 + z*(15.0 - 6.0*z)), pz = z + z3*(-6.0 + z*(8.0 - 3.0*z)),
//         o_0 = e, o_k = smin(hi_{n_k}, smax(lo_{n_k}, e*qz + (g0*D)*pz))
//     points (per node): P_0 = (X0 + rx, Y0 + ry), P_k = (x_{n_k} + o_k*nx_{n_k}, y_{n_k} + o_k*ny_{n_k})
//     d' (per segment): o_k == 0.0 && o_{k+1} == 0.0 ? d_k : |P_{k+1} - P_k|
//     kappa', psi (per node): on the line (o == 0.0 at k-1, k, k+1) the row's; else Menger's
//         curvature through P_{k-1}, P_k, P_{k+1} and atan2_cr of P_{k+1} - P_{k-1}; an end node
//         off the line takes its neighbour's curvature (K >= 2) and its one segment's direction
//     ceiling, envelope, march, per query: the retime stage's, with kappa' and d'
//     ticks: tau_m = (double)m*dt; count = #{m < M_cap : tau_m < tt_K}, the rejoin stage's node
//         bisection, the columns between the nodes' P, psi, kappa', w, s and o
// raceline.recover_host states the same in NumPy, and the two agree bit for bit (heading: up to
// the rounding of the host's atan2).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_math.h"
#include "rl_recover.h"

namespace rl {

namespace {

// the nodes' arrays in LDS
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

}  // namespace

// One workgroup per query, in the retime kernel's steps with more parallel passes before the
// serial ones.  The locate is hzn_locate; all lanes stage kappa_k and r_k of the nodes k <= K
// into LDS (march_stage).  Then five passes with one node per lane, strided, a barrier after
// each: the offsets and their clamp, the points, the segments' lengths, the nodes' curvatures and
// headings, and the ceiling (which overwrites the row's curvatures: nothing reads them after the
// pass before).  Lane 0 runs the retime stage's envelope and march (retime_pass) over LDS; the
// waves count the clamped nodes and find the merge node with a butterfly each and meet in LDS.
// All lanes stride over the ticks and over the node arrays.  No atomics: every output element has
// one writer.  LDS: eleven node arrays (11 x 4 104 B).
__global__ __launch_bounds__(HZN_THREADS) void rl_recover_kernel(RcvParams cp) {
    __shared__ double s_kap[RCV_MAX_NODES + 1];    // kappa_k, then c_k
    __shared__ double s_r[RCV_MAX_NODES + 1];
    __shared__ double s_o[RCV_MAX_NODES + 1];
    __shared__ double s_px[RCV_MAX_NODES + 1];
    __shared__ double s_py[RCV_MAX_NODES + 1];
    __shared__ double s_d[RCV_MAX_NODES + 1];
    __shared__ double s_kp[RCV_MAX_NODES + 1];     // kappa'_k
    __shared__ double s_psi[RCV_MAX_NODES + 1];
    __shared__ double s_b[RCV_MAX_NODES + 1];
    __shared__ double s_w[RCV_MAX_NODES + 1];
    __shared__ double s_tt[RCV_MAX_NODES + 1];
    __shared__ uint64_t s_key[HZN_THREADS / 64];
    __shared__ uint32_t s_idx[HZN_THREADS / 64];
    __shared__ int s_cl[HZN_THREADS / 64];
    __shared__ int s_mg[HZN_THREADS / 64];
    __shared__ int s_m1;
    const RtmParams& tp = cp.rt;
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
    // the located point, by every lane: every pass needs it
    const int i0 = (int)win.idx;
    const Foot f = hzn_foot(row.x, row.y, N, i0, px, py);
    const int room = q.closed ? N : N - 1 - i0;   // >= 1: i0 < S
    int K = rp.K_cap < room ? rp.K_cap : room;
    if (K > RCV_MAX_NODES) K = RCV_MAX_NODES;     // (the entry points refuse such a K_cap: the nodes fit the LDS arrays)
    if (K < 1) {                                   // no node ahead (the same for every lane)
        if (tid == 0) march_empty(rp, k);
        return;
    }
    const March mr = march_from(row, s_kap, f, i0, N, h);
    const double d0 = mr.d0;
    // the bounds stage's rows of this query's row
    const size_t boff = (size_t)r * (size_t)N;
    const double *blo = cp.lo + boff, *bhi = cp.hi + boff, *bnx = cp.nx + boff, *bny = cp.ny + boff;
    // the car's offset, slope and merge length, by every lane
    const double root = sqrt(f.D);
    const double e = (f.dx * f.wy - f.dy * f.wx) < 0.0 ? -root : root;   // hzn_store_loc's e
    const double D = cp.merge_len[k];
    double g0 = 0.0;
    if (cp.dir) {
        const double hx = cp.dir[2 * (size_t)k], hy = cp.dir[2 * (size_t)k + 1];
        const double den = f.dx * hx + f.dy * hy, num = f.dx * hy - f.dy * hx;
        g0 = den > 0.0 ? smin(1.0, smax(-1.0, num / den)) : (num < 0.0 ? -1.0 : (num > 0.0 ? 1.0 : 0.0));
    }
    const double gD = g0 * D;
    march_stage(mr, tid, K, s_kap, s_r);
    // offsets and clamp
    int ncl = 0, mg = 0x7fffffff;
    for (int kk = tid; kk <= K; kk += HZN_THREADS) {
        if (kk == 0) {
            s_o[0] = e;
            continue;
        }
        const double a = d0 + (double)(kk - 1) * h;
        const double z = smin(1.0, a / D);
        const double z3 = (z * z) * z;
        const double qz = 1.0 + z3 * (-10.0 + z * (15.0 - 6.0 * z));
        const double pz = z + z3 * (-6.0 + z * (8.0 - 3.0 * z));
        const double raw = e * qz + gD * pz;
        const int n = march_sample(mr, kk);
        const double o = smin(bhi[n], smax(blo[n], raw));
        s_o[kk] = o;
        ncl += o != raw;
        if (z >= 1.0 && kk < mg) mg = kk;
    }
    for (int off = 32; off; off >>= 1) {
        ncl += __shfl_xor(ncl, off, 64);
        const int om = __shfl_xor(mg, off, 64);
        mg = om < mg ? om : mg;
    }
    if ((tid & 63) == 0) {
        s_cl[tid >> 6] = ncl;
        s_mg[tid >> 6] = mg;
    }
    __syncthreads();
    // points
    for (int kk = tid; kk <= K; kk += HZN_THREADS) {
        if (kk == 0) {
            const Node n0 = march_node(mr, 0);
            s_px[0] = n0.x + (f.wx - f.u * f.dx);
            s_py[0] = n0.y + (f.wy - f.u * f.dy);
        } else {
            const int n = march_sample(mr, kk);
            const double o = s_o[kk];
            s_px[kk] = row.x[n] + o * bnx[n];
            s_py[kk] = row.y[n] + o * bny[n];
        }
    }
    __syncthreads();
    // the segments' lengths
    for (int kk = tid; kk < K; kk += HZN_THREADS) {
        if (s_o[kk] == 0.0 && s_o[kk + 1] == 0.0) {
            s_d[kk] = kk == 0 ? d0 : h;
        } else {
            const double qx = s_px[kk + 1] - s_px[kk], qy = s_py[kk + 1] - s_py[kk];
            s_d[kk] = sqrt(qx * qx + qy * qy);
        }
    }
    __syncthreads();
    // the nodes' curvatures and headings
    const RcvNodes nd = {s_o, s_px, s_py, s_d, s_kap, K};
    for (int kk = tid; kk <= K; kk += HZN_THREADS) {
        s_kp[kk] = rcv_kappa(nd, kk);
        s_psi[kk] = rcv_on_line(nd, kk) ? march_node(mr, kk).psi : rcv_psi(nd, kk);
    }
    __syncthreads();
    // the ceiling, over the row's curvatures
    for (int kk = tid; kk <= K; kk += HZN_THREADS) s_kap[kk] = retime_ceiling(tp, s_kp[kk], s_r[kk]);
    __syncthreads();
    const double* s_c = s_kap;
    if (tid == 0) {
        const double v0 = rp.v0[k];
        const RtmPass ps = retime_pass(rp.cfg, v0, K, s_kp, s_r, s_c, s_b, s_w, s_tt, [&](int kk) { return s_d[kk]; });
        const double tte = ps.tt;
        const int m1 = tick_end(0, p.M_cap, [&](int m) { return (double)m * p.dt < tte; });
        const double t0 = hzn_t0([&](int i) { return tg[i]; }, i0, f.u);
        const int nk = i0 + K, c0 = nk >= N ? 1 : 0;   // nk < 2N
        hzn_store_loc(p, k, f, i0, h, t0, m1);
        rp.merge_node[k] = K;                          // end_node
        rp.overspeed[k] = ps.over;
        rp.scal[0][k] = tte;
        rp.scal[1][k] = tte - (((double)c0 * q.T[r] + tg[nk - c0 * N]) - t0);
        tp.feasible[k] = v0 <= s_b[0] ? 1 : 0;
        tp.bind_node[k] = ps.bn;
        tp.v_excess[k] = ps.ve;
        s_m1 = m1;
    } else if (tid == 64) {                            // the offsets' per-query values, off lane 0
        int cl = 0, m = 0x7fffffff;
        for (int w = 0; w < HZN_THREADS / 64; ++w) {
            cl += s_cl[w];
            m = s_mg[w] < m ? s_mg[w] : m;
        }
        const int j0 = mr.j0;
        const double lo0 = smax(blo[i0], blo[j0]), hi0 = smin(bhi[i0], bhi[j0]);
        cp.clamped[k] = cl;
        cp.merge_node[k] = m == 0x7fffffff ? -1 : m;
        cp.offtrack[k] = !(lo0 <= e && e <= hi0) ? 1 : 0;
        cp.scal[0][k] = lo0;
        cp.scal[1][k] = hi0;
    }
    __syncthreads();
    const int M = s_m1;
    const size_t nrow = (size_t)k * ((size_t)rp.K_cap + 1);
    for (int kk = tid; kk <= K; kk += HZN_THREADS) {
        rp.node_v[nrow + kk] = s_w[kk];
        rp.node_t[nrow + kk] = s_tt[kk];
        tp.node_b[nrow + kk] = s_b[kk];
        tp.node_c[nrow + kk] = s_c[kk];
        cp.node_o[nrow + kk] = s_o[kk];
        cp.node_k[nrow + kk] = s_kp[kk];
    }
    const size_t orow = (size_t)k * (size_t)p.M_cap;
    for (int m = tid; m < M; m += HZN_THREADS) {
        const double tau = (double)m * p.dt;
        int a = 0, en = K;                             // tt_a <= tau < tt_en (march_columns' bisection)
        while (en - a > 1) {
            const int mid = a + ((en - a) >> 1);
            if (s_tt[mid] <= tau) a = mid;
            else en = mid;
        }
        const double ta = s_tt[a], tb = s_tt[a + 1], wa = s_w[a], wb = s_w[a + 1];
        const double u = (tau - ta) / (tb - ta);
        const double d = s_d[a];
        const double sa = a == 0 ? ((double)i0 + f.u) * h : (double)(i0 + a) * h, sb = (double)(i0 + a + 1) * h;
        const double pa = s_psi[a];
        double dp = s_psi[a + 1] - pa;
        if (dp > M_PI) dp -= 2.0 * M_PI;
        else if (dp < -M_PI) dp += 2.0 * M_PI;
        const size_t o = orow + m;
        p.out[0][o] = sa + u * (sb - sa);
        p.out[1][o] = s_px[a] + u * (s_px[a + 1] - s_px[a]);
        p.out[2][o] = s_py[a] + u * (s_py[a + 1] - s_py[a]);
        p.out[3][o] = pa + u * dp;
        p.out[4][o] = s_kp[a] + u * (s_kp[a + 1] - s_kp[a]);
        p.out[5][o] = wa + u * (wb - wa);
        p.out[6][o] = d > 0.0 ? (wb * wb - wa * wa) / (2.0 * d) : 0.0;
        cp.offset[o] = s_o[a] + u * (s_o[a + 1] - s_o[a]);
    }
}

hipError_t launch_recover(const RcvParams& p, hipStream_t st) {
    hipLaunchKernelGGL(rl_recover_kernel, dim3((unsigned)p.rt.rj.hz.Q), dim3(HZN_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace rl
