// rl_stop.hip — the stop stage's kernel: "I am at (px, py) doing v0, with these
// limits, and must do v_target when I reach sample J: what do I drive until then, can I make it,
// and where does the stop start to bind?"  The rejoin stage's query (rl_rejoin.hip, §3m) with a
// target.  Per query, in fp64 without contraction:
//     locate, nodes: the rejoin stage's: seg = i, u, e, dist2, t0, s0; kappa_k, r_k, d_k, n_k = i + k, K_lim
//     target: K_s = closed ? ((J - i - 1) mod N + N) mod N + 1 : J - i; K_s < 1 or K_s > K_lim:
//         stop_node = -1, count = 0, the location still written
//     envelope (serial, backward): b_{K_s} = v_target; for k = K_s - 1 .. 0:
//         (., a_brk) = ax_max_at(cfg, b_{k+1}, kappa_{k+1}), b_k = sqrt(smax(0.0, b_{k+1}*b_{k+1} + (2.0*a_brk)*d_k))
//         reachable = v0 <= b_0
//     march (serial, forward, always to K_s): w_0 = v0, tt_0 = 0.0; for k = 0 .. K_s - 1:
//         (a_acc, a_brk) = ax_max_at(cfg, w_k, kappa_k)
//         up = sqrt(smax(0.0, w_k*w_k + (2.0*a_acc)*d_k)), dn = sqrt(smax(0.0, w_k*w_k - (2.0*a_brk)*d_k))
//         w_{k+1} = smin(up, w_k <= b_k ? smin(b_{k+1}, smax(dn, r_{k+1})) : smax(dn, smin(b_{k+1}, r_{k+1})))
//         tt_{k+1} = tt_k + (2.0*d_k)/smax(1e-6, w_k + w_{k+1})
//     per query: g_k = smin(b_k, r_k); overspeed = #{k <= K_s : w_k > g_k}, v_excess the largest
//         w_k - g_k or 0.0; brake_node the first k with b_k < r_k (none: K_s); t_stop = tt_{K_s},
//         v_end = w_{K_s}, s_stop = (double)n_{K_s}*h
//     ticks: tau_m = (double)m*dt; count = #{m < M_cap : tau_m < tt_{K_s}}, all of them on the
//         march, with the rejoin stage's node bisection and march-tick columns
// raceline.stop_host states the same in NumPy, and the two agree bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_stop.h"

namespace rl {

// One workgroup per query, in the rejoin kernel's steps with two serial passes in the middle.
// The locate is hzn_locate.  All lanes then stage kappa_k and r_k of the nodes k <= K_s into
// LDS; lane 0 sweeps the envelope backward and marches forward over them, writes b_k, w_k and
// tt_k beside them and hands K_s and the tick count over through LDS; all lanes stride over the
// ticks (consecutive lanes, consecutive ticks) and over the nodes' w, tt, b for the node arrays.
// No atomics: every output element has one writer.  Only the two stamps of the located segment
// are needed (t0); they come from global memory.  LDS: five node arrays (5 x 8 200 B).
__global__ __launch_bounds__(HZN_THREADS) void rl_stop_kernel(StpParams sp) {
    __shared__ double s_kap[RJN_MAX_NODES + 1];
    __shared__ double s_r[RJN_MAX_NODES + 1];
    __shared__ double s_b[RJN_MAX_NODES + 1];
    __shared__ double s_w[RJN_MAX_NODES + 1];
    __shared__ double s_tt[RJN_MAX_NODES + 1];
    __shared__ uint64_t s_key[HZN_THREADS / 64];
    __shared__ uint32_t s_idx[HZN_THREADS / 64];
    __shared__ int s_m1;
    const RjnParams& rp = sp.rj;
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
    // no stamps in LDS (the horizon and rejoin kernels stage them): only t0 reads two, from here
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
    const int K_lim = rp.K_cap < room ? rp.K_cap : room;
    // the target node: the first time sample J comes up ahead of the located segment (the entry
    // points refuse a J outside [0, N); the test here only keeps a launch that skipped them from
    // indexing LDS with it)
    const int J = sp.stop_sample[k];
    int Ks = -1;
    if (J >= 0 && J < N) Ks = q.closed ? ((J - i0 - 1) % N + N) % N + 1 : J - i0;
    const bool in_range = Ks >= 1 && Ks <= K_lim;  // K_lim <= RJN_MAX_NODES: the nodes fit the LDS arrays
    // the location first: a target out of range still answers where the car is.  These are
    // hzn_store_loc's stores and hzn_t0's formula written out: a store helper without the count
    // (the count stored by the callers), one for the sign of e alone, and hzn_t0 here were each
    // compiled, and each changed the register allocation of this kernel or of the other two
    if (tid == 0) {
        const double ta0 = tg[i0];
        const double root = sqrt(f.D);
        p.seg[k] = i0;
        p.loc[0][k] = f.u;
        p.loc[1][k] = ta0 + f.u * (tg[i0 + 1] - ta0);
        p.loc[2][k] = ((double)i0 + f.u) * h;
        p.loc[3][k] = (f.dx * f.wy - f.dy * f.wx) < 0.0 ? -root : root;
        p.loc[4][k] = f.D;
        if (!in_range) {
            p.count[k] = 0;
            rp.merge_node[k] = -1;
        }
    }
    if (!in_range) return;                         // (the same for every lane)
    const March mr = march_from(row, s_kap, f, i0, N, h);
    const double d0 = mr.d0;
    march_stage(mr, tid, Ks, s_kap, s_r);
    __syncthreads();
    if (tid == 0) {
        const double v0 = rp.v0[k];
        double e = sp.v_target[k];                 // the envelope, backward from the target
        s_b[Ks] = e;
        for (int kk = Ks - 1; kk >= 0; --kk) {
            const double d = kk == 0 ? d0 : h;
            const AxMax a = ax_max_at(rp.cfg, e, s_kap[kk + 1]);
            e = sqrt(smax(0.0, e * e + (2.0 * a.brk) * d));
            s_b[kk] = e;
        }
        double w = v0, tt = 0.0, ve = 0.0;         // the march, forward to the target
        int over = 0, bn = -1;
        s_w[0] = w;
        s_tt[0] = 0.0;
        for (int kk = 0;; ++kk) {
            const double bk = s_b[kk], rk = s_r[kk];
            const double g = smin(bk, rk);
            over += w > g;
            ve = smax(ve, w - g);
            if (bn < 0 && bk < rk) bn = kk;
            if (kk == Ks) break;
            const double d = kk == 0 ? d0 : h;
            const Reach s = march_step(rp.cfg, w, s_kap[kk], d);
            const double bn1 = s_b[kk + 1], rn = s_r[kk + 1];
            const double wn = smin(s.up, w <= bk ? smin(bn1, smax(s.dn, rn)) : smax(s.dn, smin(bn1, rn)));
            tt = march_time(tt, d, w, wn);
            s_w[kk + 1] = wn;
            s_tt[kk + 1] = tt;
            w = wn;
        }
        // the first m with !(tau_m < tt_{K_s}): tick_end's loop, written out here because through
        // the helper the compiler orders this kernel's two selects the other way round
        int a = 0, m = p.M_cap;
        while (a < m) {
            const int mid = a + ((m - a) >> 1);
            if ((double)mid * p.dt < tt) a = mid + 1;
            else m = mid;
        }
        p.count[k] = a;
        rp.merge_node[k] = Ks;
        rp.overspeed[k] = over;
        rp.scal[0][k] = tt;
        rp.scal[1][k] = w;
        sp.reachable[k] = v0 <= s_b[0] ? 1 : 0;
        sp.brake_node[k] = bn < 0 ? Ks : bn;
        sp.scal[0][k] = (double)(i0 + Ks) * h;
        sp.scal[1][k] = ve;
        s_m1 = a;
    }
    __syncthreads();
    const int M = s_m1;
    const size_t nrow = (size_t)k * ((size_t)rp.K_cap + 1);
    for (int kk = tid; kk <= Ks; kk += HZN_THREADS) {
        rp.node_v[nrow + kk] = s_w[kk];
        rp.node_t[nrow + kk] = s_tt[kk];
        sp.node_b[nrow + kk] = s_b[kk];
    }
    const size_t orow = (size_t)k * (size_t)p.M_cap;
    for (int m = tid; m < M; m += HZN_THREADS) march_columns(p, mr, s_w, s_tt, Ks, (double)m * p.dt, orow + m);
}

hipError_t launch_stop(const StpParams& p, hipStream_t st) {
    hipLaunchKernelGGL(rl_stop_kernel, dim3((unsigned)p.rj.hz.Q), dim3(HZN_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace rl
