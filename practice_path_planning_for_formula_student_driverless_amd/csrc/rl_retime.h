// rl_retime.h — launch interface of the retime stage's kernel (rl_retime.hip): the
// rejoin stage's query answered with the reference's forward/backward speed pass over the nodes
// ahead of the car, under the query's cfg: a ceiling per node, a brake envelope swept backward
// under it, the car's speed marched forward under that, and the ticks along the march
// (rl_stages.cpp rl_plan_retime, rl_abi.cpp rl_retime).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_rejoin.h"

namespace rl {

constexpr int RTM_SCAL = 1;             // v_excess: the double beyond the rejoin stage's two
constexpr int RTM_INTS = 2;             // feasible, bind_node: the ints beyond the rejoin stage's four
constexpr int RTM_NODES = 2;            // node_b, node_c: the node arrays beyond the rejoin stage's two

struct RtmParams {
    // the rejoin stage's query and outputs as launch_rejoin takes them.  Four of its outputs
    // carry the retime stage's: merge_node is end_node, overspeed is overspeed, scal[0] is
    // t_end, scal[1] is t_loss; node_v, node_t are the march's w, tt.
    RjnParams rj;
    double v_cap, a_lat_max, kappa_eps;   // the ceiling's cfg fields, copied
    int32_t* feasible;             // [Q]
    int32_t* bind_node;            // [Q]
    double* v_excess;              // [Q]
    double* node_b;                // [Q][K_cap + 1]
    double* node_c;                // [Q][K_cap + 1]
};
// one workgroup per query; the conditions of launch_rejoin
hipError_t launch_retime(const RtmParams& p, hipStream_t st);

// ------------------------------------------------------------------ shared device functions
// the ceiling of a node of curvature kap on a row that drives it at r (§3p "ceiling")
__device__ __forceinline__ double retime_ceiling(const RtmParams& tp, double kap, double r) {
    const double vk = sqrt(tp.a_lat_max / smax(fabs(kap), tp.kappa_eps));
    return smin(smin(tp.v_cap, vk), r);
}

// The serial passes of §3p by the calling lane, over the nodes 0 .. K in LDS (the recover
// stage's kernel, rl_recover.hip, runs them on its own geometry): the envelope s_b swept backward
// under the ceiling s_c, then v0 marched forward under it into s_w, s_tt; dist(k) is d_k.
// Returns the march's time at K, overspeed, v_excess and bind_node.
struct RtmPass {
    double tt, ve;
    int over, bn;
};
template <class Dist>
__device__ __forceinline__ RtmPass retime_pass(const RjnCfg& cfg, double v0, int K, const double* s_kap, const double* s_r,
                                               const double* s_c, double* s_b, double* s_w, double* s_tt, const Dist& dist) {
    double e = s_c[K];                             // the envelope, backward from the last node
    s_b[K] = e;
    for (int kk = K - 1; kk >= 0; --kk) {
        const double d = dist(kk);
        const AxMax a = ax_max_at(cfg, e, s_kap[kk + 1]);
        e = smin(s_c[kk], sqrt(smax(0.0, e * e + (2.0 * a.brk) * d)));
        s_b[kk] = e;
    }
    double w = v0, tt = 0.0, ve = 0.0;             // the march, forward to the last node
    int over = 0, bn = -1;
    s_w[0] = w;
    s_tt[0] = 0.0;
    for (int kk = 0;; ++kk) {
        const double bk = s_b[kk];
        over += w > bk;
        ve = smax(ve, w - bk);
        if (bn < 0 && bk < s_r[kk]) bn = kk;
        if (kk == K) break;
        const double d = dist(kk);
        const Reach s = march_step(cfg, w, s_kap[kk], d);
        const double bn1 = s_b[kk + 1];
        const double wn = smin(s.up, w <= bk ? bn1 : smax(s.dn, bn1));
        tt = march_time(tt, d, w, wn);
        s_w[kk + 1] = wn;
        s_tt[kk + 1] = tt;
        w = wn;
    }
    return {tt, ve, over, bn};
}

}  // namespace rl
