// rl_select.h — launch interface of the selection stage (rl_select.hip): score the
// instances of a batch, rank them per group and gather the winners' rows, all on the
// device (rl_stages.cpp rl_plan_select, rl_abi.cpp rl_rank_scores).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rl {

// score[b] = h * sum_i kappa[b][i]^2, h = (Ls ? Ls[b] : L) / N  (N >= 1, B >= 1)
hipError_t launch_score(const double* kappa, int32_t N, int32_t B, double L, const double* Ls, double* score,
                        hipStream_t st);

// B = G * group_size instances in G contiguous groups; index[G][k] = the global indices of
// the k best of each group, best first, ascending in (isnan(score), score, index);
// score_sel[G][k] = score[index] (may be nullptr).  1 <= k <= min(group_size, 64).
hipError_t launch_rank(const double* score, int32_t B, int32_t group_size, int32_t k, int32_t* index,
                       double* score_sel, hipStream_t st);

// The result arrays of one mode, as sources [B][.] and compact destinations [rows][.];
// a nullptr source or destination skips the array.
constexpr int RL_SEL_F64 = 8;               // x, y, heading, kappa, alpha_total, alpha_last, v, ax
struct GatherParams {
    const double* src[RL_SEL_F64];          // [B][N]
    double* dst[RL_SEL_F64];                // [rows][N]
    const double* lap_src;                  // [B]
    double* lap_dst;                        // [rows]
    const int32_t *evals_src, *accepts_src, *sweeps_src;   // [B][mo], [B][mo], [B][mo + 1]
    int32_t *evals_dst, *accepts_dst, *sweeps_dst;
    const int32_t* index;                   // [rows], every entry in [0, B)
    int32_t N, B, mo, rows;
};
hipError_t launch_gather(const GatherParams& g, hipStream_t st);

}  // namespace rl
