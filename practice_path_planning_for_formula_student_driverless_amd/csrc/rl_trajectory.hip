// rl_trajectory.hip — the trajectory stage's kernel: a raceline sampled every h
// metres becomes what a controller tracks, the state at every control tick.  Per row
//     t_0 = 0,  t_{i+1} = t_i + h / smax(1e-6, v_i)       (ref:854-860, added in index order)
//     T = t_S,  S = closed ? N : N - 1 segments, segment i from sample i to (i + 1) mod N
//     tick m at tau_m = (double)m * dt,  M = min(M_cap, #{m : tau_m < T})  (0 for a NaN / inf T)
//     its segment: the i in [0, S) with t_i <= tau_m < t_{i+1},  u = (tau_m - t_i) / (t_{i+1} - t_i)
//     s = (i + u) * h;  x, y, v, kappa = a_i + u * (a_j - a_i);  ax = ax_i (constant on a
//     segment, ref:858);  heading = psi_i + u * d, d = psi_j - psi_i moved into [-pi, pi]
// in fp64 without contraction: raceline.trajectory_host states the same in NumPy, and the two
// agree bit for bit.  For closed rows T is the reference's lap summed serially; the optimiser's
// own `lap` is a tree sum of the same terms and may differ from it in the last bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_trajectory.h"

namespace rl {

// One workgroup per output row: TRAJ_T worker lanes and one more wave whose lane 0 adds.
//
// Phase A, the stamps, follows rl_path_prep_kernel (rl_lap_stage.hip): tile j covers samples
// [j * TRAJ_T, (j + 1) * TRAJ_T); the workers write h / smax(1e-6, v_i) of tile j + 1 into one
// LDS buffer (coalesced loads of v) while the adding lane walks tile j in the other, in index
// order, and leaves every partial sum t_{i+1} in s_t; one barrier per tile hands the buffers
// over.  The workers copy tile j - 1's stamps to the global row in the same step (consecutive
// lanes, consecutive addresses).  Rows of N <= TRAJ_LDS_N samples keep all N + 1 stamps in s_t;
// longer rows use its first two tiles as a ring and read the stamps back from the global row:
// the storing lanes fence, the workgroup meets at a barrier, then everyone loads.
//
// Phase B, the ticks: the adding lane finds M by bisection over m (m -> (double)m * dt is
// monotone, so #{m : tau_m < T} is the first m that fails the test); then all lanes stride
// over m, each finds its segment by bisection over the stamps with the comparisons above, and
// writes its seven values (consecutive lanes, consecutive ticks).  No atomics: every output
// element has one writer.
constexpr int TRAJ_T = 256;
constexpr int TRAJ_THREADS = TRAJ_T + 64;
static_assert((TRAJ_T & (TRAJ_T - 1)) == 0 && TRAJ_LDS_N + 1 >= 2 * TRAJ_T, "ring of two tiles inside s_t");

__global__ __launch_bounds__(TRAJ_THREADS) void rl_trajectory_kernel(TrajParams q) {
    __shared__ double s_d[2][TRAJ_T];
    __shared__ double s_t[TRAJ_LDS_N + 1];
    __shared__ int s_M;
    const int r = blockIdx.x, tid = threadIdx.x, N = q.N;
    const int b = q.index ? q.index[r] : r;
    if (b < 0 || b >= q.B) {                      // not an instance: no ticks, nothing else
        if (tid == 0) q.count[r] = 0;
        return;
    }
    double* tg = q.stamps + (size_t)r * ((size_t)N + 1);
    if (N == 0) {
        if (tid == 0) {
            tg[0] = 0.0;
            q.T[r] = 0.0;
            q.count[r] = 0;
        }
        return;
    }
    const size_t off = (size_t)b * (size_t)N;
    const double* v = q.v + off;
    const double h = q.h ? q.h[b] : (q.Ls ? q.Ls[b] : q.L) / (double)N;
    const int S = q.closed ? N : N - 1;
    const bool lds = N <= TRAJ_LDS_N;
    const int ntiles = (N + TRAJ_T - 1) / TRAJ_T;
    const bool worker = tid < TRAJ_T;
    auto slot = [&](int k) { return lds ? k : (k & (2 * TRAJ_T - 1)); };
    auto fill = [&](int j) {
        const int i = j * TRAJ_T + tid;
        if (i < N) s_d[j & 1][tid] = h / smax(1e-6, v[i]);
    };
    auto flush = [&](int j) {
        const int i = j * TRAJ_T + tid;
        if (i < N) tg[i + 1] = s_t[slot(i + 1)];
    };
    if (tid == 0) tg[0] = 0.0;
    if (worker) fill(0);
    __syncthreads();
    double t = 0.0, tp = 0.0;                     // t_{i+1} and t_i of the adding lane
    for (int j = 0; j < ntiles; ++j) {
        if (worker) {
            if (j + 1 < ntiles) fill(j + 1);
            if (j > 0) flush(j - 1);
        } else if (tid == TRAJ_T) {
            const int base = j * TRAJ_T, cnt = min(TRAJ_T, N - base);
            const double* d = s_d[j & 1];
            if (j == 0) s_t[0] = 0.0;
            for (int k = 0; k < cnt; ++k) {
                tp = t;
                t = t + d[k];
                s_t[slot(base + k + 1)] = t;
            }
            if (j + 1 == ntiles) {
                const double T = q.closed ? t : tp;            // t_S
                int lo = 0, hi = q.M_cap;                      // the first m with !(tau_m < T)
                while (lo < hi) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if ((double)mid * q.dt < T) lo = mid + 1;
                    else hi = mid;
                }
                const int M = __builtin_isfinite(T) ? lo : 0;
                s_M = M;
                q.T[r] = T;
                q.count[r] = M;
            }
        }
        __syncthreads();
    }
    if (worker) flush(ntiles - 1);
    if (!lds) {
        // the ticks read stamps that other lanes of this workgroup stored to the global row
        __threadfence();
        __syncthreads();
    }
    const int M = s_M;
    auto stamp = [&](int k) { return lds ? s_t[k] : tg[k]; };
    const double* x = q.x + off;
    const double* y = q.y + off;
    const double* psi = q.heading + off;
    const double* kap = q.kappa + off;
    const double* ax = q.ax + off;
    const size_t orow = (size_t)r * (size_t)q.M_cap;
    for (int m = tid; m < M; m += TRAJ_THREADS) {
        const double tau = (double)m * q.dt;
        int lo = 0, hi = S;                       // t_lo <= tau < t_hi  (t_0 = 0 <= tau < T = t_S)
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (stamp(mid) <= tau) lo = mid;
            else hi = mid;
        }
        const int i = lo, jn = i + 1 < N ? i + 1 : 0;
        const double t0 = stamp(i), t1 = stamp(i + 1);
        const double u = (tau - t0) / (t1 - t0);
        const double xi = x[i], yi = y[i], vi = v[i], ki = kap[i], pi = psi[i];
        double d = psi[jn] - pi;
        if (d > M_PI) d -= 2.0 * M_PI;
        else if (d < -M_PI) d += 2.0 * M_PI;
        q.out[0][orow + m] = ((double)i + u) * h;
        q.out[1][orow + m] = xi + u * (x[jn] - xi);
        q.out[2][orow + m] = yi + u * (y[jn] - yi);
        q.out[3][orow + m] = pi + u * d;
        q.out[4][orow + m] = ki + u * (kap[jn] - ki);
        q.out[5][orow + m] = vi + u * (v[jn] - vi);
        q.out[6][orow + m] = ax[i];
    }
}

hipError_t launch_trajectory(const TrajParams& q, hipStream_t st) {
    hipLaunchKernelGGL(rl_trajectory_kernel, dim3((unsigned)q.R), dim3(TRAJ_THREADS), 0, st, q);
    return hipGetLastError();
}

}  // namespace rl
