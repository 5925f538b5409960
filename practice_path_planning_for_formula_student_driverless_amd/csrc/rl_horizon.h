// rl_horizon.h — launch interface of the horizon stage's kernel (rl_horizon.hip):
// query poses are located on rows of a trajectory stage and the next ticks from there are
// resampled, across the start line on closed rows (rl_stages.cpp rl_plan_horizon, rl_abi.cpp
// rl_horizon).  Below it, the device functions of that kernel which the rejoin and stop stages'
// kernels (rl_rejoin.hip; rl_stop.hip, §3n) share: the query's row, the empty answer,
// the parallel locate, the located point and its stores, the tick count's bisection and a tick's
// wrap and columns.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_trajectory.h"

namespace rl {

constexpr int HZN_LOC = 5;              // u, t0, s0, e, dist2 (rl_hzn's order)

struct HznParams {
    // the trajectory stage whose rows are queried, as it was launched: its source rows, step,
    // index, stamps [R][N + 1] and T [R] are read; its columns and counts are not touched
    TrajParams src;
    const double* pose;        // [Q][2]
    const int32_t* row;        // [Q] row of the trajectory stage; nullptr: 0
    const int32_t* hint;       // [Q] segment hint, -1 = every segment; nullptr: all -1
    double* out[TRAJ_COLS];    // [Q][M_cap] each
    double* loc[HZN_LOC];      // [Q] each
    int32_t* seg;              // [Q]
    int32_t* count;            // [Q]
    double dt;
    int32_t Q, window, M_cap;
};
// one workgroup per query; Q >= 1, window >= 0, 1 <= M_cap, dt > 0, src.N >= 1
hipError_t launch_horizon(const HznParams& p, hipStream_t st);

// ------------------------------------------------------------------ shared device functions
constexpr int HZN_THREADS = 256;
// order keys of D: a D that is not NaN is >= +0, so its bits order as it does; every NaN takes
// one key above +inf's (the index then decides among them); a lane without a candidate loses
// every comparison
constexpr uint64_t HZN_KEY_NAN = 0x7ff8000000000000ull;
constexpr uint64_t HZN_KEY_NONE = ~0ull;
constexpr uint32_t HZN_IDX_NONE = 0xffffffffu;

__device__ __forceinline__ bool key_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
    return ka < kb || (ka == kb && ia < ib);
}

// the pose's nearest point on one segment: its parameter u and squared distance D
struct Foot {
    double dx, dy, wx, wy, u, D;
};
__device__ __forceinline__ Foot foot(double xi, double yi, double xj, double yj, double px, double py) {
    Foot f;
    f.dx = xj - xi;
    f.dy = yj - yi;
    f.wx = px - xi;
    f.wy = py - yi;
    const double dd = f.dx * f.dx + f.dy * f.dy;
    const double c = f.wx * f.dx + f.wy * f.dy;
    f.u = dd > 0.0 ? smin(1.0, smax(0.0, c / dd)) : 0.0;
    const double rx = f.wx - f.u * f.dx, ry = f.wy - f.u * f.dy;
    f.D = rx * rx + ry * ry;
    return f;
}

// The parallel locate of query k by a workgroup of HZN_THREADS lanes: the lanes stride over the
// candidates and each keeps its least (key, index); the wave folds its 64 with an xor butterfly,
// the waves meet in LDS (s_key, s_idx: one slot per wave) and every lane reads all slots
// (rl_rank_kernel's scheme).  Every lane returns the winner (key, idx); key >= HZN_KEY_NAN or
// idx >= S: a NaN winner, or no candidate at all.  Holds one barrier, which also publishes what
// the lanes wrote to LDS before the call.
struct HznWin {
    uint64_t key;
    uint32_t idx;
};
// The candidates of a hint g (-1: every segment) and window W on a row of S segments: lo + c,
// c in [0, C), taken mod S on a closed row (lo > -S, lo + C < 2S).  The rollout stage's chain
// (rl_rollout.hip) takes its candidates from here too.
struct HznRange {
    int lo, C;
};
__device__ __forceinline__ HznRange hzn_range(int closed, int S, int g, int64_t W) {
    int lo = 0, C = S;
    if (g >= 0) {
        if (closed) {
            if (2 * W + 1 < (int64_t)S) {
                lo = g % S - (int)W;
                C = 2 * (int)W + 1;
            }
        } else {
            const int64_t a = (int64_t)g - W, e = (int64_t)g + W;
            lo = (int)(a < 0 ? 0 : a);
            C = (int)(e > S - 1 ? S - 1 : e) - lo + 1;         // <= 0 for a hint past the row: no candidate
        }
    }
    return {lo, C};
}
__device__ __forceinline__ HznWin hzn_locate(const HznParams& p, int k, int tid, const double* x, const double* y,
                                             double px, double py, uint64_t* s_key, uint32_t* s_idx) {
    const TrajParams& q = p.src;
    const int N = q.N;
    const int S = q.closed ? N : N - 1;
    const HznRange rg = hzn_range(q.closed, S, p.hint ? p.hint[k] : -1, p.window);
    const int lo = rg.lo, C = rg.C;
    uint64_t bk = HZN_KEY_NONE;
    uint32_t bi = HZN_IDX_NONE;
    for (int c = tid; c < C; c += HZN_THREADS) {
        int i = lo + c;
        if (i < 0) i += S;
        else if (i >= S) i -= S;
        const int j = i + 1 < N ? i + 1 : 0;
        const double D = foot(x[i], y[i], x[j], y[j], px, py).D;
        const uint64_t key = D != D ? HZN_KEY_NAN : (uint64_t)__double_as_longlong(D);
        if (key_less(key, (uint32_t)i, bk, bi)) {
            bk = key;
            bi = (uint32_t)i;
        }
    }
    for (int o = 32; o; o >>= 1) {
        const uint64_t ok = __shfl_xor(bk, o, 64);
        const uint32_t oi = __shfl_xor(bi, o, 64);
        if (key_less(ok, oi, bk, bi)) {
            bk = ok;
            bi = oi;
        }
    }
    if ((tid & 63) == 0) {
        s_key[tid >> 6] = bk;
        s_idx[tid >> 6] = bi;
    }
    __syncthreads();
    bk = s_key[0];
    bi = s_idx[0];
    for (int w = 1; w < HZN_THREADS / 64; ++w) {
        const uint64_t ok = s_key[w];
        const uint32_t oi = s_idx[w];
        if (key_less(ok, oi, bk, bi)) {
            bk = ok;
            bi = oi;
        }
    }
    return {bk, bi};
}

// a tick's time tau on a row of lap T: the wrap count c and the row time w (§3l "ticks")
struct HznLap {
    double c, w;
};
__device__ __forceinline__ HznLap hzn_wrap(int closed, double T, double tau) {
    double c = 0.0, w = tau;
    if (closed) {
        c = floor(tau / T);
        w = tau - c * T;
        if (w < 0.0) {
            w += T;
            c -= 1.0;
        } else if (w >= T) {
            w -= T;
            c += 1.0;
        }
    }
    return {c, w};
}

// the segment of row time w: §3k's bisection on w over stamp(0 .. S) (the bounds stage's tick
// kernel, rl_bounds.hip, takes its segments from here too)
template <class Stamp>
__device__ __forceinline__ int hzn_segment(const Stamp& stamp, int S, double w) {
    int a = 0, e = S;                          // t_a <= w < t_e on a sorted row; clipped otherwise
    while (e - a > 1) {
        const int mid = a + ((e - a) >> 1);
        if (stamp(mid) <= w) a = mid;
        else e = mid;
    }
    return a;
}

// the source rows of one instance, and a tick's seven columns at row time w in lap c, written to
// element o of p.out: hzn_segment's segment, then §3l's columns
struct HznRow {
    const double *x, *y, *psi, *kap, *v, *ax;
};
template <class Stamp>
__device__ __forceinline__ void hzn_columns(const HznParams& p, const HznRow& r, const Stamp& stamp, int N, int S,
                                            double h, double c, double w, size_t o) {
    const int i = hzn_segment(stamp, S, w), jn = i + 1 < N ? i + 1 : 0;
    const double ta = stamp(i), tb = stamp(i + 1);
    const double u = (w - ta) / (tb - ta);
    const double xi = r.x[i], yi = r.y[i], vi = r.v[i], ki = r.kap[i], pi = r.psi[i];
    double d = r.psi[jn] - pi;
    if (d > M_PI) d -= 2.0 * M_PI;
    else if (d < -M_PI) d += 2.0 * M_PI;
    p.out[0][o] = ((c * (double)S + (double)i) + u) * h;
    p.out[1][o] = xi + u * (r.x[jn] - xi);
    p.out[2][o] = yi + u * (r.y[jn] - yi);
    p.out[3][o] = pi + u * d;
    p.out[4][o] = ki + u * (r.kap[jn] - ki);
    p.out[5][o] = vi + u * (r.v[jn] - vi);
    p.out[6][o] = r.ax[i];
}

// The row of query k: the instance of row r of the trajectory stage, -1 for an r outside the
// stage (the caller also refuses an instance outside the batch and a row without a segment); its
// source rows, its stamps in global memory and its step
__device__ __forceinline__ int hzn_instance(const TrajParams& q, int r) {
    int b = -1;
    if (r >= 0 && r < q.R) b = q.index ? q.index[r] : r;
    return b;
}
__device__ __forceinline__ HznRow hzn_row(const TrajParams& q, int b) {
    const size_t off = (size_t)b * (size_t)q.N;
    return {q.x + off, q.y + off, q.heading + off, q.kappa + off, q.v + off, q.ax + off};
}
__device__ __forceinline__ const double* hzn_stamps(const TrajParams& q, int r) {
    return q.stamps + (size_t)r * ((size_t)q.N + 1);
}
__device__ __forceinline__ double hzn_step(const TrajParams& q, int b) {
    return q.h ? q.h[b] : (q.Ls ? q.Ls[b] : q.L) / (double)q.N;
}

// the answer of a query without a row or without a winner, by the calling lane
__device__ __forceinline__ void hzn_empty(const HznParams& p, int k) {
    p.seg[k] = -1;
    p.count[k] = 0;
}

// the located point: the pose's foot on the winning segment i0, and its time on the row
__device__ __forceinline__ Foot hzn_foot(const double* x, const double* y, int N, int i0, double px, double py) {
    const int j0 = i0 + 1 < N ? i0 + 1 : 0;
    return foot(x[i0], y[i0], x[j0], y[j0], px, py);
}
template <class Stamp>
__device__ __forceinline__ double hzn_t0(const Stamp& stamp, int i0, double u) {
    const double ta = stamp(i0);
    return ta + u * (stamp(i0 + 1) - ta);
}
// seg, count and the five location fields of query k, by the calling lane (§3l "location")
__device__ __forceinline__ void hzn_store_loc(const HznParams& p, int k, const Foot& f, int i0, double h, double t0,
                                              int cnt) {
    const double root = sqrt(f.D);
    p.seg[k] = i0;
    p.count[k] = cnt;
    p.loc[0][k] = f.u;
    p.loc[1][k] = t0;
    p.loc[2][k] = ((double)i0 + f.u) * h;
    p.loc[3][k] = (f.dx * f.wy - f.dy * f.wx) < 0.0 ? -root : root;
    p.loc[4][k] = f.D;
}

// the first m in [a, M_cap] with !before(m), for a `before` that is monotone in m: a tick count
template <class Before>
__device__ __forceinline__ int tick_end(int a, int M_cap, const Before& before) {
    int e = M_cap;
    while (a < e) {
        const int mid = a + ((e - a) >> 1);
        if (before(mid)) a = mid + 1;
        else e = mid;
    }
    return a;
}

}  // namespace rl
