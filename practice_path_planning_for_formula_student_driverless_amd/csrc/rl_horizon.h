// rl_horizon.h — launch interface of the horizon stage's kernel (rl_horizon.hip):
// query poses are located on rows of a trajectory stage and the next ticks from there are
// resampled, across the start line on closed rows (rl_stages.cpp rl_plan_horizon, rl_abi.cpp
// rl_horizon).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_trajectory.h"

namespace rl {

constexpr int HZN_LOC = 5;              // u, t0, s0, e, dist2 (rl_hzn's order)

struct HznParams {
    // the trajectory stage whose rows are queried, as it was launched: its source rows, step,
    // index, stamps [R][N + 1] and T [R] are read; its columns and counts are not touched
    TrajParams src;
    const double* pose;        // [Q][2]
    const int32_t* row;        // [Q] row of the trajectory stage; nullptr: 0
    const int32_t* hint;       // [Q] segment hint, -1 = every segment; nullptr: all -1
    double* out[TRAJ_COLS];    // [Q][M_cap] each
    double* loc[HZN_LOC];      // [Q] each
    int32_t* seg;              // [Q]
    int32_t* count;            // [Q]
    double dt;
    int32_t Q, window, M_cap;
};
// one workgroup per query; Q >= 1, window >= 0, 1 <= M_cap, dt > 0, src.N >= 1
hipError_t launch_horizon(const HznParams& p, hipStream_t st);

}  // namespace rl
