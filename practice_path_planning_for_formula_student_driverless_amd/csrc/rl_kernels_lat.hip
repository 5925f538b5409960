// rl_kernels_lat.hip — the latency shapes of the register-resident optimiser kernel
// (rl_optimize_body.h): one instance spread over a whole CU with 1-4 samples per lane.
//
// The reference's own use is one track per call (pipeline::compute_raceline_and_save
// ref:1347, compute_mintime_and_save ref:1397): a batch of one leaves 255 of 256 CUs idle,
// and the throughput shapes' per-lane serial work (4-8 samples per lane, one or four
// waves) sets the latency.  Spreading the instance over 4-16 waves cuts each lane's
// chain of dependent fp64 operations per evaluation at the price of the cross-wave
// reductions and exchanges (LDS + barriers).  pick_shape (rl_kernels.hip) selects these
// shapes while the batch needs at most one wave per SIMD in them.  Results equal the
// throughput shapes' bit for bit except the lap sum's tree order (the same kernel
// template; every per-sample expression and every J / decrease sum is the same).
// The (4, 512) shape has a translation unit of its own (rl_kernels_mid.hip) so that each
// can be compiled with the instruction scheduler that suits it (build.py TU_FLAGS).
#include "rl_optimize_body.h"

namespace rl {

#ifdef RL_STAMPS
// diagnostic builds: this translation unit's copy of the per-phase cycle totals
int debug_stamps_lat(unsigned long long* host, int nblocks) { return read_stamps(rl_dbg_stamps, host, nblocks); }
#endif

hipError_t launch_optimize_lat(const KParams& p, const Shape& s, bool mintime, hipStream_t st) {
    if (p.N <= 0 || p.N > s.K * s.T) return hipErrorInvalidValue;
    RL_SHAPES_LAT(RL_LAUNCH_IF)
    return launch_optimize_mid(p, s, mintime, st);       // (4, 512): rl_kernels_mid.hip
}

}  // namespace rl
