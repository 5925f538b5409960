// rl_lap_stage.h — launch interface of the lap stage's preparation kernel
// (rl_lap_stage.hip): the result rows of a plan become the inputs of a lap evaluation
// (rl_stages.cpp rl_plan_lap, rl_abi.cpp rl_path_lengths).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_abi.h"

namespace rl {

struct PrepParams {
    const double* x;           // [B][N] result rows (SoA)
    const double* y;           // [B][N]
    double* centre;            // [B][N][2] packed paths, or nullptr (path lengths only)
    double* L_out;             // [B] path lengths, summed in index order (closing term last)
    const rl_cfg* cfg_src;     // [ncfg] the plan's cfgs, or nullptr
    rl_cfg* cfg_dst;           // [ncfg] copies with max_outer_iters = 0
    int32_t N, B, closed, ncfg;
};
// one workgroup per instance; N >= 0, B >= 1
hipError_t launch_path_prep(const PrepParams& q, hipStream_t st);

}  // namespace rl
