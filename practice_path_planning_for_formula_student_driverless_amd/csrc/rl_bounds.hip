// rl_bounds.hip — the bounds stage's kernels: "how much room do I have on either
// side?", answered about the raceline itself.  Every tick of the trajectory, horizon, rejoin and
// stop stages carries s, x, y, heading, kappa, v, ax and the location carries the lateral offset
// e; these kernels add the free track width that e may use.  In fp64 without contraction.
//
// rl_bounds_kernel, per row r of the trajectory stage (instance b = index[r], points P_i =
// (x[b][i], y[b][i])) and sample i:
//     normal: normals_from_points_generic (ref:581-593) as rl_corridor_kernel states it: N == 1:
//         t = (1, 0); closed rows: t = (P_{i+1} - P_{i-1})*0.5 across the start line; open rows:
//         t = P_1 - P_0 at i = 0, P_{N-1} - P_{N-2} at i = N - 1, the same central difference
//         between; sqrt(tx*tx + ty*ty) < 1e-15: t = (1, 0); n = (-ty, tx)/|.| (0 if |.| < 1e-15),
//         so +n is left of travel, the sign of the horizon stage's e
//     bounds: corridor_bounds<2> (rl_corridor.h) with guard = veh_width*0.5 + margin:
//         hi = max(0, dpos - guard), lo = -max(0, dneg - guard), the reference's safe_ray block
//         (ref:692-711); the same device code as every other corridor of the library
// rl_horizon_bounds_kernel, per query q of the horizon stage (row r, located segment seg, t0,
// count) and tick m < count: tau_m = t0 + (double)m*dt, the horizon stage's wrap (c, w) and its
// bisection on w give the segment i, j = (i + 1) mod N, and
//     lo_m = smax(lo_i, lo_j), hi_m = smin(hi_i, hi_j):
// the conservative pair of the segment's two samples, never looser than either, no rounding.
// lo0, hi0 are that pair of seg.  A query with seg = -1 writes nothing.
// raceline.normals_host and raceline.horizon_bounds_host state the new pieces in NumPy.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rl_bounds.h"
#include "rl_corridor.h"
#include "rl_device.h"

namespace rl {

// rl_corridor_kernel's mapping (rl_geom.hip), batched: each lane takes CK = 2 adjacent samples,
// a workgroup of 256 lanes 512 consecutive samples of one row, blockIdx.y the row (rows beyond
// the grid's y extent are taken in turn).  The casts are corridor_bounds<2>, whose ring reads
// are uniform in a wave: a wave lies in one row.  No LDS, no barrier; every output element has
// one writer.
__global__ __launch_bounds__(256) void rl_bounds_kernel(BndParams p) {
    constexpr int CK = 2;
    const int N = p.N;
    const int i0 = (blockIdx.x * blockDim.x + threadIdx.x) * CK;
    for (int r = blockIdx.y; r < p.R; r += gridDim.y) {
        const int b = p.index ? p.index[r] : r;
        if (b < 0 || b >= p.B) continue;            // (no such instance: the row stays as it was)
        const double* X = p.x + (size_t)b * (size_t)N;
        const double* Y = p.y + (size_t)b * (size_t)N;
        double qx[CK], qy[CK], ux[CK], uy[CK], lo[CK], hi[CK];
        bool act[CK];
#pragma unroll
        for (int k = 0; k < CK; ++k) {
            const int i = min(i0 + k, N - 1);
            act[k] = i0 + k < N;
            double tx, ty;
            if (N == 1) { tx = 1; ty = 0; }
            else if (p.closed) {
                const int ip = (i + 1 == N) ? 0 : i + 1, im = (i == 0) ? N - 1 : i - 1;
                tx = (X[ip] - X[im]) * 0.5; ty = (Y[ip] - Y[im]) * 0.5;
            } else if (i == 0) { tx = X[1] - X[0]; ty = Y[1] - Y[0]; }
            else if (i == N - 1) { tx = X[N - 1] - X[N - 2]; ty = Y[N - 1] - Y[N - 2]; }
            else { tx = (X[i + 1] - X[i - 1]) * 0.5; ty = (Y[i + 1] - Y[i - 1]) * 0.5; }
            if (sqrt(tx * tx + ty * ty) < 1e-15) { tx = 1; ty = 0; }
            const double vx = -ty, vy = tx, n = sqrt(vx * vx + vy * vy);   // geom::normalize ref:132
            ux[k] = 0.0; uy[k] = 0.0;
            if (!(n < 1e-15)) { ux[k] = vx / n; uy[k] = vy / n; }
            qx[k] = X[i];
            qy[k] = Y[i];
        }
        corridor_bounds<CK>(p.ring[0], p.ring[1], qx, qy, ux, uy, act, p.guard, lo, hi);
        const size_t o = (size_t)r * (size_t)N + (size_t)i0;
#pragma unroll
        for (int k = 0; k < CK; ++k)
            if (act[k]) {
                p.lo[o + k] = lo[k];
                p.hi[o + k] = hi[k];
                p.nx[o + k] = ux[k];
                p.ny[o + k] = uy[k];
            }
    }
}

hipError_t launch_bounds(const BndParams& p, hipStream_t st) {
    if (p.N <= 0 || p.R <= 0) return hipSuccess;
    const int T = 256, per = T * 2;
    const dim3 grid((unsigned)((p.N + per - 1) / per), (unsigned)(p.R < 65535 ? p.R : 65535));
    hipLaunchKernelGGL(rl_bounds_kernel, grid, dim3(T), 0, st, p);
    return hipGetLastError();
}

// One workgroup per query of the horizon stage, the lanes striding over its ticks as that
// stage's kernel does (consecutive lanes, consecutive ticks).  It reads what that kernel left
// in HBM (seg, t0, count) and the stamps of the trajectory stage's row; nothing is uploaded.
__global__ __launch_bounds__(HZN_THREADS) void rl_horizon_bounds_kernel(HznBndParams p) {
    const HznParams& z = p.hz;
    const TrajParams& q = z.src;
    const int k = blockIdx.x, tid = threadIdx.x, N = q.N;
    const int S = q.closed ? N : N - 1;
    const int r = z.row ? z.row[k] : 0;
    const int seg = z.seg[k];
    if (seg < 0 || seg >= S || r < 0 || r >= q.R) return;   // not located: nothing is specified
    const double* lo = p.lo + (size_t)r * (size_t)N;
    const double* hi = p.hi + (size_t)r * (size_t)N;
    if (tid == 0) {
        const int j = seg + 1 < N ? seg + 1 : 0;
        p.lo0[k] = smax(lo[seg], lo[j]);
        p.hi0[k] = smin(hi[seg], hi[j]);
    }
    const int M = min(z.count[k], z.M_cap);
    const double* tg = q.stamps + (size_t)r * ((size_t)N + 1);
    auto stamp = [&](int i) { return tg[i]; };
    const double T = q.T[r], t0 = z.loc[1][k];
    const size_t orow = (size_t)k * (size_t)z.M_cap;
    for (int m = tid; m < M; m += HZN_THREADS) {
        const HznLap l = hzn_wrap(q.closed, T, t0 + (double)m * z.dt);
        const int i = hzn_segment(stamp, S, l.w), j = i + 1 < N ? i + 1 : 0;
        p.tlo[orow + m] = smax(lo[i], lo[j]);
        p.thi[orow + m] = smin(hi[i], hi[j]);
    }
}

hipError_t launch_horizon_bounds(const HznBndParams& p, hipStream_t st) {
    if (p.hz.Q <= 0) return hipSuccess;
    hipLaunchKernelGGL(rl_horizon_bounds_kernel, dim3((unsigned)p.hz.Q), dim3(HZN_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace rl
