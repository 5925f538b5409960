// rl_trajectory.h — launch interface of the trajectory stage's kernel (rl_trajectory.hip,
// DESIGN §3k): result rows x, y, heading, kappa, v, ax [B][N] sampled every h metres become
// time-stamped trajectories sampled every dt seconds (rl_stages.cpp rl_plan_trajectory,
// rl_abi.cpp rl_trajectory).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rl {

constexpr int TRAJ_COLS = 7;            // s, x, y, heading, kappa, v, ax (rl_traj's order)
// rows of at most this many samples keep their stamps in LDS for the tick phase (the
// register-resident optimiser's range); longer rows read them back from the global row
constexpr int TRAJ_LDS_N = 4096;

struct TrajParams {
    const double *x, *y, *heading, *kappa, *v, *ax;   // [B][N] source rows (SoA)
    // the step of instance b: h[b] if h is given, else Ls[b] / N if Ls is given, else L / N
    const double* h;
    const double* Ls;
    double L;
    const int32_t* index;      // [R] output row r reads instance index[r]; nullptr: r itself
    double* out[TRAJ_COLS];    // [R][M_cap] each
    double* stamps;            // [R][N + 1]
    double* T;                 // [R]
    int32_t* count;            // [R]
    double dt;
    int32_t N, B, R, closed, M_cap;
};
// one workgroup per output row; N >= 0, B >= 1, R >= 1, 1 <= M_cap, dt > 0
hipError_t launch_trajectory(const TrajParams& q, hipStream_t st);

}  // namespace rl
