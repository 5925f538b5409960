// rl_kernels.hip — MI355X (gfx950) batched raceline optimizer, steps 7-8 of the
// reference pipeline (ref = /root/reference/src/main.cpp): the throughput shapes of the
// register-resident kernel (rl_optimize_body.h) and the launch dispatch by (N, B).
// The latency shapes for small batches are instantiated in rl_kernels_lat.hip.
#include <cstdlib>

#include "rl_optimize_body.h"

namespace rl {

#ifdef RL_STAMPS
int debug_stamps(unsigned long long* host, int nblocks) { return read_stamps(rl_dbg_stamps, host, nblocks); }
#endif

// (the shape tables by N: rl_kernels.h THR_SHAPES / LAT_SHAPES)
static_assert(RL_MID_K * RL_MID_T == 2048, "mid variant must cover N <= 2048");
static_assert(RL_MIDMT_K == 4 && RL_MIDMT_T == 512, "the mid min-time shape is (4, 512), instantiated in rl_kernels_mid.hip");

static int cu_count() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return 256;
    return n > 0 ? n : 256;
}

bool lat_shapes_enabled() {
    const char* e = std::getenv("RL_LAT_SHAPES");
    return !(e && e[0] == '0');
}

Shape pick_shape(int N, int B, bool mintime, int cus) {
    if (N <= 0 || N > RL_REG_MAX_N) return {-1, -1};
    const Shape lat = fit_shape(LAT_SHAPES, N);
    if (lat.K > 0 && lat_shapes_enabled() && (int64_t)B * (lat.T / 64) <= (int64_t)4 * cus) return lat;
    const Shape s = fit_shape(THR_SHAPES, N);
    // min-time, 1024 < N <= 2048: (4, 512) holds one instance per CU (8 waves at 2 waves/SIMD),
    // the lower latency while the batch leaves CUs idle; from two instances per CU up, the
    // (RL_MID_K, RL_MID_T) shape keeps two per CU resident for throughput
    if (s == Shape{RL_MID_K, RL_MID_T} && mintime && B < 2 * cus) return {RL_MIDMT_K, RL_MIDMT_T};
    return s;
}

#ifdef RL_COUNT
// diagnostic builds: this translation unit's corridor counters (the throughput shapes)
int debug_counts_reg(unsigned long long* host, int reset) { return read_counts(rl_dbg_count, host, reset); }
#endif

hipError_t launch_optimize(const KParams& p, bool mintime, hipStream_t st) {
    if (p.N <= 0 || fit_shape(THR_SHAPES, p.N).K < 0) return hipErrorInvalidValue;
#ifdef RL_ANALYZE_ONE   // static analysis builds (scripts/regs_one.sh): the C2/C3 shape only (2: open)
    constexpr bool CL = RL_ANALYZE_ONE != 2;
    return mintime ? launch_shape<8, 256, CL, true>(p, st) : launch_shape<8, 256, CL, false>(p, st);
#else
    const Shape s = pick_shape(p.N, p.shape_B > 0 ? p.shape_B : p.B, mintime, cu_count());
    // (the mid row fans out by mode first: the order its kernels have in the code object)
#define RL_LAUNCH_MID_IF(K_, T_) \
    if (s == Shape{K_, T_}) return mintime ? launch_shape<K_, T_, true>(p, st) : launch_shape<K_, T_, false>(p, st);
    RL_SHAPES_THR(RL_LAUNCH_IF, RL_LAUNCH_MID_IF)
#undef RL_LAUNCH_MID_IF
    return launch_optimize_lat(p, s, mintime, st);
#endif
}

}  // namespace rl
