// rl_recover.h — launch interface of the recover stage's kernel (rl_recover.hip): the
// rejoin stage's query with a merge length and the car's direction, answered with a lateral
// offset profile from the car's offset to zero inside the bounds stage's free width, the
// geometry of that offset path, the retime stage's speed pass on it and the ticks along it
// (rl_stages.cpp rl_plan_recover, rl_abi.cpp rl_recover).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace rl
