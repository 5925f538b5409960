// rl_bounds.h — launch interface of the bounds stage's two kernels (rl_bounds.hip):
// the free track width about every sample of the trajectory stage's rows, cast with the corridor
// code of the optimisers (rl_corridor.h) from the rows as they lie in HBM, and the same at the
// horizon stage's ticks (rl_stages.cpp rl_plan_bounds and rl_plan_horizon_bounds, rl_abi.cpp
// rl_bounds).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_corridor.h"
#include "rl_horizon.h"

namespace rl {

struct BndParams {
    const double *x, *y;       // [B][N] source rows (SoA), the trajectory stage's
    const int32_t* index;      // [R] bounds row r reads instance index[r]; nullptr: r itself
    RingDesc ring[2];          // inner, outer ring as entry streams
    double guard;              // veh_width * 0.5 + margin
    double *lo, *hi, *nx, *ny; // [R][N] each
    int32_t N, B, R, closed;
};
// 512 consecutive samples of one row per workgroup; N >= 1, R >= 1
hipError_t launch_bounds(const BndParams& p, hipStream_t st);

struct HznBndParams {
    // the horizon stage as it was launched: its src (stamps, T, N, R, closed), row, seg, loc[1]
    // (t0), count, dt, Q and M_cap are read; nothing of it is written
    HznParams hz;
    const double *lo, *hi;     // [R][N] the bounds stage's rows of the same trajectory stage
    double *tlo, *thi;         // [Q][M_cap]
    double *lo0, *hi0;         // [Q]
};
// one workgroup per query
hipError_t launch_horizon_bounds(const HznBndParams& p, hipStream_t st);

}  // namespace rl
