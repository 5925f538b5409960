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

}  // namespace rl
