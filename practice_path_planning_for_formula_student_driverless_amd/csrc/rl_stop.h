// rl_stop.h — launch interface of the stop stage's kernel (rl_stop.hip): the rejoin
// stage's query with a target, "be at v_target when you reach sample J": a brake envelope is
// swept backward from the target, the car's speed is marched forward under it, and the ticks
// follow the march up to the target (rl_stages.cpp rl_plan_stop, rl_abi.cpp rl_stop).  Not part
// of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_rejoin.h"

namespace rl {

constexpr int STP_SCAL = 2;             // s_stop, v_excess: the doubles beyond the rejoin stage's two
constexpr int STP_INTS = 2;             // reachable, brake_node: the ints beyond the rejoin stage's four

struct StpParams {
    // the rejoin stage's query and outputs as launch_rejoin takes them.  Four of its outputs
    // carry the stop stage's: merge_node is stop_node, overspeed is overspeed, scal[0] is
    // t_stop, scal[1] is v_end; node_v, node_t are the march's w, tt.
    RjnParams rj;
    const int32_t* stop_sample;    // [Q]
    const double* v_target;        // [Q]
    int32_t* reachable;            // [Q]
    int32_t* brake_node;           // [Q]
    double* scal[STP_SCAL];        // [Q] each
    double* node_b;                // [Q][K_cap + 1]
};
// one workgroup per query; the conditions of launch_rejoin, and 0 <= stop_sample[q] < src.N
hipError_t launch_stop(const StpParams& p, hipStream_t st);

}  // namespace rl
