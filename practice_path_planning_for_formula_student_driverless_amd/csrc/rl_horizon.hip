// rl_horizon.hip — the horizon stage's kernel: a controller's question, "I am at
// (px, py); where on the raceline is that, and what are the next M ticks from there?", answered
// for Q poses on rows of the last trajectory stage (rl_trajectory.hip, §3k), whose samples,
// step h, stamps t_0 .. t_N and T = t_S it reads as they lie in HBM.  Per query, in fp64
// without contraction (S = closed ? N : N - 1 segments, segment i from sample i to j = (i + 1) mod N):
//     candidates: every i in [0, S) without a hint; with a hint g and window W the segments
//         (g + k) mod S, k = -W .. W, of a closed row (all of them if 2W + 1 >= S), and
//         max(0, g - W) .. min(S - 1, g + W) of an open one
//     distance: dx = x_j - x_i, dy = y_j - y_i, wx = px - x_i, wy = py - y_i, dd = dx*dx + dy*dy,
//         c = wx*dx + wy*dy, u = dd > 0 ? smin(1, smax(0, c/dd)) : 0, rx = wx - u*dx,
//         ry = wy - u*dy, D = rx*rx + ry*ry
//     winner: the candidate least in (isnan(D), D, i); a NaN winner or S = 0: seg = -1, count = 0
//     location: seg = i, u, dist2 = D, e = (dx*wy - dy*wx) < 0 ? -sqrt(D) : sqrt(D),
//         t0 = t_i + u*(t_{i+1} - t_i), s0 = ((double)i + u)*h
//     ticks: tau_m = t0 + (double)m*dt.  Open rows: count = min(M_cap, #{m : tau_m < T}), c = 0,
//         w = tau_m.  Closed rows: count = M_cap if T is finite and > 0, else 0; c = floor(tau_m/T),
//         w = tau_m - c*T, then at most one fix-up each way (w < 0: w += T, c -= 1; else
//         w >= T: w -= T, c += 1).  Segment of a tick: §3k's bisection on w; u_m = (w - t_i) /
//         (t_{i+1} - t_i); s = ((c*(double)S + (double)i) + u_m)*h; the other six columns are §3k's.
// raceline.horizon_host states the same in NumPy, and the two agree bit for bit: each D depends
// on its own segment only, so the shape of the reduction does not show in the result.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_horizon.h"

namespace rl {

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

// One workgroup per query.  The lanes stride over the candidates and each keeps its least
// (key, index); the wave folds its 64 with an xor butterfly, the waves meet in LDS and every
// lane reads all slots (rl_rank_kernel's scheme).  The same barrier publishes the stamps of a
// row of N <= TRAJ_LDS_N samples, which the lanes copied into LDS on the way; longer rows read
// the trajectory stage's global row.  Lane 0 computes the location and the tick count and hands
// t0 and the count over through LDS; then all lanes stride over m (consecutive lanes,
// consecutive ticks).  No atomics: every output element has one writer.
__global__ __launch_bounds__(HZN_THREADS) void rl_horizon_kernel(HznParams p) {
    __shared__ double s_t[TRAJ_LDS_N + 1];
    __shared__ uint64_t s_key[HZN_THREADS / 64];
    __shared__ uint32_t s_idx[HZN_THREADS / 64];
    __shared__ double s_t0;
    __shared__ int s_count;
    const TrajParams& q = p.src;
    const int k = blockIdx.x, tid = threadIdx.x, N = q.N;
    const int S = q.closed ? N : N - 1;
    const int r = p.row ? p.row[k] : 0;
    int b = -1;
    if (r >= 0 && r < q.R) b = q.index ? q.index[r] : r;
    if (b < 0 || b >= q.B || S < 1) {             // no row, or a row without a segment
        if (tid == 0) {
            p.seg[k] = -1;
            p.count[k] = 0;
        }
        return;
    }
    const size_t off = (size_t)b * (size_t)N;
    const double* x = q.x + off;
    const double* y = q.y + off;
    const double* tg = q.stamps + (size_t)r * ((size_t)N + 1);
    const bool lds = N <= TRAJ_LDS_N;
    if (lds)
        for (int i = tid; i <= N; i += HZN_THREADS) s_t[i] = tg[i];
    const double px = p.pose[2 * (size_t)k], py = p.pose[2 * (size_t)k + 1];

    // the candidates are lo + c, c in [0, C), taken mod S on a closed row (lo > -S, lo + C < 2S)
    const int g = p.hint ? p.hint[k] : -1;
    const int64_t W = p.window;
    int lo = 0, C = S;
    if (g >= 0) {
        if (q.closed) {
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
    if (bk >= HZN_KEY_NAN || bi >= (uint32_t)S) {  // a NaN winner, or no candidate at all
        if (tid == 0) {
            p.seg[k] = -1;
            p.count[k] = 0;
        }
        return;
    }
    auto stamp = [&](int i) { return lds ? s_t[i] : tg[i]; };
    const double h = q.h ? q.h[b] : (q.Ls ? q.Ls[b] : q.L) / (double)N;
    const double T = q.T[r];
    if (tid == 0) {
        const int i = (int)bi, j = i + 1 < N ? i + 1 : 0;
        const Foot f = foot(x[i], y[i], x[j], y[j], px, py);
        const double ta = stamp(i);
        const double t0 = ta + f.u * (stamp(i + 1) - ta);
        const double root = sqrt(f.D);
        int cnt;
        if (q.closed) {
            cnt = (__builtin_isfinite(T) && T > 0.0) ? p.M_cap : 0;
        } else {
            int a = 0, e = p.M_cap;                // the first m with !(tau_m < T)
            while (a < e) {
                const int mid = a + ((e - a) >> 1);
                if (t0 + (double)mid * p.dt < T) a = mid + 1;
                else e = mid;
            }
            cnt = a;
        }
        p.seg[k] = i;
        p.count[k] = cnt;
        p.loc[0][k] = f.u;
        p.loc[1][k] = t0;
        p.loc[2][k] = ((double)i + f.u) * h;
        p.loc[3][k] = (f.dx * f.wy - f.dy * f.wx) < 0.0 ? -root : root;
        p.loc[4][k] = f.D;
        s_t0 = t0;
        s_count = cnt;
    }
    __syncthreads();
    const double t0 = s_t0;
    const int M = s_count;
    const double* psi = q.heading + off;
    const double* kap = q.kappa + off;
    const double* v = q.v + off;
    const double* ax = q.ax + off;
    const size_t orow = (size_t)k * (size_t)p.M_cap;
    for (int m = tid; m < M; m += HZN_THREADS) {
        const double tau = t0 + (double)m * p.dt;
        double c = 0.0, w = tau;
        if (q.closed) {
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
        int a = 0, e = S;                          // t_a <= w < t_e on a sorted row; clipped otherwise
        while (e - a > 1) {
            const int mid = a + ((e - a) >> 1);
            if (stamp(mid) <= w) a = mid;
            else e = mid;
        }
        const int i = a, jn = i + 1 < N ? i + 1 : 0;
        const double ta = stamp(i), tb = stamp(i + 1);
        const double u = (w - ta) / (tb - ta);
        const double xi = x[i], yi = y[i], vi = v[i], ki = kap[i], pi = psi[i];
        double d = psi[jn] - pi;
        if (d > M_PI) d -= 2.0 * M_PI;
        else if (d < -M_PI) d += 2.0 * M_PI;
        p.out[0][orow + m] = ((c * (double)S + (double)i) + u) * h;
        p.out[1][orow + m] = xi + u * (x[jn] - xi);
        p.out[2][orow + m] = yi + u * (y[jn] - yi);
        p.out[3][orow + m] = pi + u * d;
        p.out[4][orow + m] = ki + u * (kap[jn] - ki);
        p.out[5][orow + m] = vi + u * (v[jn] - vi);
        p.out[6][orow + m] = ax[i];
    }
}

hipError_t launch_horizon(const HznParams& p, hipStream_t st) {
    hipLaunchKernelGGL(rl_horizon_kernel, dim3((unsigned)p.Q), dim3(HZN_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace rl
