// rl_rollout.h — launch interface of the rollout stage's kernel (rl_rollout.hip):
// Q sampled trajectories of T poses each are located pose by pose on rows of the last trajectory
// stage, every pose's hint the segment found for the pose before it, and scored against the row,
// its speed profile and the bounds stage's free width (rl_stages.cpp rl_plan_rollouts, rl_abi.cpp
// rl_rollouts).  The ranking of the costs is rl_select.h's launch_rank.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_trajectory.h"

namespace rl {

constexpr int RLL_POSE_F64 = 6;         // u, e, dist2, s, margin, vref (rl_rll's order)
constexpr int RLL_HEAD_F64 = 4;         // progress, e_max, margin_min, cost
constexpr int RLL_HEAD_I32 = 3;         // count, valid, first_out

struct RllParams {
    // the trajectory stage whose rows are queried, as it was launched: its x, y, v, step, index,
    // N, B, R and closed are read; nothing of it is written
    TrajParams src;
    const double *lo, *hi;     // [R][N] the bounds stage's rows of the same trajectory stage
    const double* xy;          // [Q][T][2]
    const double* v;           // [Q][T]; nullptr: no speed term
    const int32_t* row;        // [Q] row of the trajectory stage; nullptr: 0
    const int32_t* hint;       // [Q] segment hint of pose 0, -1 = every segment; nullptr: all -1
    int32_t* seg;              // [Q][T]
    double* pose[RLL_POSE_F64];   // [Q][T] each
    double* head[RLL_HEAD_F64];   // [Q] each
    int32_t* ihead[RLL_HEAD_I32]; // [Q] each
    double w_e, w_out, w_v, w_prog;
    int32_t Q, T, window0, window, hard_bounds;
};
// one wave per rollout, four rollouts per workgroup; Q >= 1, T >= 1, windows >= 0
hipError_t launch_rollouts(const RllParams& p, hipStream_t st);

}  // namespace rl
