// rl_recover_fan.h — launch interface of the fan stage's kernels (rl_recover_fan.hip):
// the recover stage's query with C merge lengths per pose.  Every candidate is the recover
// stage's answer for its length; the candidates of a pose are ranked in the exact order
// (class, isnan(t_end), t_end, index) and the first one's results, ticks and node arrays are the
// stage's, with a table of the candidates' per-query values (rl_stages.cpp rl_plan_recover_fan,
// rl_abi.cpp rl_recover_fan).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_recover.h"

namespace rl {

constexpr int FAN_MAX_CAND = 16;        // RL_FAN_MAX_CAND
constexpr int FAN_TAB_INTS = 6;         // cand_class, cand_feasible, cand_clamped, cand_merge_node, cand_overspeed, cand_bind_node
constexpr int FAN_TAB_SCAL = 3;         // cand_t_end, cand_t_loss, cand_v_excess
constexpr int FAN_XNODES = 4;           // P.x, P.y, d', psi: the node arrays of a candidate beyond the recover stage's six

struct FanParams {
    // the stage's results, the winners': a recover launch of Q queries, whose query pointers are
    // the fan's (pose, v0, row, hint, dir [Q]; merge_len [Q][C])
    RcvParams win;
    // the candidates' results in the scratch block: a recover launch of Q*C queries without
    // ticks (its columns and offset are not written) on the same query pointers
    RcvParams cand;
    double* xnode[FAN_XNODES];     // scratch, [Q*C][K_cap + 1] each
    int32_t C;
    int32_t* best;                 // [Q]
    int32_t* tab_i[FAN_TAB_INTS];  // [Q][C] each
    double* tab_d[FAN_TAB_SCAL];   // [Q][C] each
};
// the candidate kernel, one workgroup per candidate, then the select kernel, one per query, on the
// same stream; the conditions of launch_recover, 1 <= C <= FAN_MAX_CAND
hipError_t launch_recover_fan(const FanParams& p, hipStream_t st);

}  // namespace rl
