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

// One workgroup per query, in the retime kernel's steps with more parallel passes before the
// serial ones.  The locate is hzn_locate; all lanes stage kappa_k and r_k of the nodes k <= K
// into LDS (march_stage).  Then five passes with one node per lane, strided, a barrier after
// each: the offsets and their clamp, the points, the segments' lengths, the nodes' curvatures and
// headings, and the ceiling (which overwrites the row's curvatures: nothing reads them after the
// pass before).  Lane 0 runs the retime stage's envelope and march (retime_pass) over LDS; the
// waves count the clamped nodes and find the merge node with a butterfly each and meet in LDS.
// All lanes stride over the ticks and over the node arrays.  No atomics: every output element has
// one writer.  LDS: eleven node arrays (11 x 4 104 B).  The phases are rl_recover.h's device
// functions (rcv_solve and rcv_tick), which the fan stage's kernels share.
__global__ __launch_bounds__(HZN_THREADS) void rl_recover_kernel(RcvParams cp) {
    __shared__ RcvShared sh;
    const RtmParams& tp = cp.rt;
    const RjnParams& rp = tp.rj;
    const HznParams& p = rp.hz;
    const int k = blockIdx.x, tid = threadIdx.x;
    RcvGeo g;
    if (!rcv_solve(cp, k, k, k, tid, sh, g)) return;
    const int K = g.K, M = sh.m1;
    const double* s_c = sh.kap;
    const size_t nrow = (size_t)k * ((size_t)rp.K_cap + 1);
    for (int kk = tid; kk <= K; kk += HZN_THREADS) {
        rp.node_v[nrow + kk] = sh.w[kk];
        rp.node_t[nrow + kk] = sh.tt[kk];
        tp.node_b[nrow + kk] = sh.b[kk];
        tp.node_c[nrow + kk] = s_c[kk];
        cp.node_o[nrow + kk] = sh.o[kk];
        cp.node_k[nrow + kk] = sh.kp[kk];
    }
    const RcvTicks nt = {sh.o, sh.px, sh.py, sh.d, sh.kp, sh.psi, sh.w, sh.tt, g.f.u, g.h, g.i0, K};
    const size_t orow = (size_t)k * (size_t)p.M_cap;
    for (int m = tid; m < M; m += HZN_THREADS) rcv_tick(cp, nt, (double)m * p.dt, orow + m);
}

hipError_t launch_recover(const RcvParams& p, hipStream_t st) {
    hipLaunchKernelGGL(rl_recover_kernel, dim3((unsigned)p.rt.rj.hz.Q), dim3(HZN_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace rl
