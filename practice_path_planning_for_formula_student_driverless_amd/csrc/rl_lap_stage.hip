// rl_lap_stage.hip — the lap stage's preparation kernel: the SoA result rows
// x[b][.], y[b][.] of a plan become the inputs of a lap evaluation, the interleaved path
// [B][N][2] and its own length L_mc[b], without leaving the device.  The evaluation itself
// is the min-time kernel at max_outer_iters = 0 (rl_stages.cpp rl_plan_lap), launched as
// rl_lap_eval launches it; this file holds no second v-pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_lap_stage.h"
#include "rl_math.h"

namespace rl {

// One workgroup per instance: PREP_T worker lanes and one more wave whose lane 0 sums.
// Tile j covers samples [j * PREP_T, (j + 1) * PREP_T).  A worker lane packs its sample
// (one 16-byte store per lane, consecutive lanes consecutive addresses; the x and y loads
// are coalesced too) and writes its segment length
//     d_i = hypot_ref(x[i+1] - x[i], y[i+1] - y[i])          (i < N-1)
//     d_{N-1} = hypot_ref(x[0] - x[N-1], y[0] - y[N-1])      (closed tracks)
// into the tile's LDS buffer.  The length is the debug dump's path_length (ref:1443-1448):
//     L = (((0.0 + d_0) + d_1) + ...) in index order, the closing term last,
// so the sum is a serial chain by contract: the summing lane adds tile j's entries in order
// while the workers fill tile j + 1 into the other buffer; one barrier per tile hands the
// buffers over.  No atomics and no tree: L's bits depend on the row alone.  N <= 1: 0.0.
constexpr int PREP_T = 256;

__global__ __launch_bounds__(PREP_T + 64) void rl_path_prep_kernel(PrepParams q) {
    __shared__ double s_d[2][PREP_T];
    const int b = blockIdx.x, tid = threadIdx.x, N = q.N;
    const size_t off = (size_t)b * (size_t)N;
    const double* x = q.x + off;
    const double* y = q.y + off;
    double2* cen = q.centre ? reinterpret_cast<double2*>(q.centre) + off : nullptr;
    const int nseg = N <= 1 ? 0 : (q.closed ? N : N - 1);
    const int ntiles = (N + PREP_T - 1) / PREP_T;
    const bool worker = tid < PREP_T;
    // the evaluation's cfgs: the plan's, with no optimiser iteration
    if (tid == 0 && q.cfg_src && b < q.ncfg) {
        rl_cfg c = q.cfg_src[b];
        c.max_outer_iters = 0;
        q.cfg_dst[b] = c;
    }
    auto fill = [&](int j) {
        const int i = j * PREP_T + tid;
        if (i >= N) return;
        const double xi = x[i], yi = y[i];
        if (cen) cen[i] = make_double2(xi, yi);
        if (i < nseg) {
            const int n = i + 1 < N ? i + 1 : 0;
            s_d[j & 1][tid] = hypot_ref(x[n] - xi, y[n] - yi);
        }
    };
    if (worker && ntiles > 0) fill(0);
    __syncthreads();
    double tot = 0.0;
    for (int j = 0; j < ntiles; ++j) {
        if (worker) {
            if (j + 1 < ntiles) fill(j + 1);
        } else if (tid == PREP_T) {
            // (an open track whose N - 1 is a multiple of the tile leaves the last tile empty)
            const int cnt = min(PREP_T, nseg - j * PREP_T);
            const double* d = s_d[j & 1];
            for (int k = 0; k < cnt; ++k) tot = tot + d[k];
        }
        __syncthreads();
    }
    if (tid == PREP_T) q.L_out[b] = tot;
}

hipError_t launch_path_prep(const PrepParams& q, hipStream_t st) {
    hipLaunchKernelGGL(rl_path_prep_kernel, dim3((unsigned)q.B), dim3(PREP_T + 64), 0, st, q);
    return hipGetLastError();
}

}  // namespace rl
