// rl_rejoin.h — launch interface of the rejoin stage's kernel (rl_rejoin.hip): the
// horizon stage's query with the car's speed and limits: a reachable speed profile is marched
// from the located point until it meets the row's own, and the ticks follow it (rl_stages.cpp
// rl_plan_rejoin, rl_abi.cpp rl_rejoin).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
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

}  // namespace rl
