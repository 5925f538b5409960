// rl_kernels_mid.hip — the (4, 512) shape of the register-resident optimiser kernel
// (rl_optimize_body.h): the latency shape for 1024 < N <= 2048 and the min-time shape for
// that N range below two instances per CU (rl_kernels.hip pick_shape).  A translation unit
// of its own so that it can be compiled with its own instruction scheduler (build.py
// TU_FLAGS; A/B in DESIGN.md §3e).
#include "rl_optimize_body.h"

namespace rl {

#ifdef RL_STAMPS
// diagnostic builds: this translation unit's copy of the per-phase cycle totals
int debug_stamps_mid(unsigned long long* host, int nblocks) { return read_stamps(rl_dbg_stamps, host, nblocks); }
#endif

hipError_t launch_optimize_mid(const KParams& p, const Shape& s, bool mintime, hipStream_t st) {
    if (p.N <= 1024 || p.N > 2048) return hipErrorInvalidValue;
    RL_SHAPE_MID4(RL_LAUNCH_IF)
    return hipErrorInvalidValue;
}

}  // namespace rl
