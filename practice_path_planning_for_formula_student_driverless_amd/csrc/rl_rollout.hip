// rl_rollout.hip — the rollout stage's kernel: a sampling controller's question,
// "here are Q short trajectories of T poses each; how far does each get along the raceline, how
// far off it does it stray, does it leave the free width, how does its speed compare with the
// plan's?", answered on rows of the last trajectory stage (rl_trajectory.hip, §3k) and the bounds
// stage's rows of the same (rl_bounds.hip, §3o).  Per rollout, in fp64 without contraction
// (S = closed ? N : N - 1 segments, segment i from sample i to j = (i + 1) mod N, h the row's step):
//     chain: pose 0 is located as the horizon stage (§3l) locates a pose with hint seg_hint and
//         window window0; pose t >= 1 with hint seg_{t-1} and window `window`: the same candidates,
//         the same distance, the same least (isnan(D), D, i).  The first pose without a winner (a
//         NaN winner or no candidate) ends the chain: count = t, and the poses from t on hold NaN
//         and seg = -1.  A rollout without a row, or on a row without a segment: count = 0.
//     pose: seg, u, dist2 = D and e = (dx*wy - dy*wx) < 0 ? -sqrt(D) : sqrt(D) as §3l's location;
//         c_0 = 0 and on a closed row, with d = seg_t - seg_{t-1}: c_t = c_{t-1} + 1 if 2d < -S,
//         c_{t-1} - 1 if 2d > S, c_{t-1} otherwise (open rows: 0);
//         s = (((double)c*(double)S + (double)seg) + u)*h;
//         lo_t = smax(lo_i, lo_j), hi_t = smin(hi_i, hi_j) (§3o's pair), margin = smin(hi_t - e, e - lo_t);
//         vref = v_i + u*(v_j - v_i)
//     rollout, over the located poses in ascending t, every sum from 0.0: E = sum e*e,
//         O = sum (margin < 0 ? margin*margin : 0.0), V = sum (v_t - vref)*(v_t - vref) (no v: 0.0),
//         e_max = smax(e_max, |e|) from 0.0, margin_min = smin(margin_min, margin) from +inf,
//         first_out = the first t with margin < 0 (none: T); valid = (count == T);
//         progress = s_{T-1} - s_0 and cost = ((w_e*E + w_out*O) + w_v*V) - w_prog*progress, +inf in
//         its place if hard_bounds and first_out < T; both NaN unless valid
// raceline.rollouts_host states the same in NumPy, and the two agree bit for bit: each D depends
// on its own segment only and the sums are added in the specification's order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_horizon.h"
#include "rl_rollout.h"

namespace rl {

constexpr int RLL_THREADS = 256;
constexpr int RLL_WAVES = RLL_THREADS / 64;

// lane l's value of v, l uniform in the wave: two scalar lane reads, no LDS
__device__ __forceinline__ double lane_f64(double v, int l) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// One wave per rollout, four rollouts per workgroup; the waves share nothing, so there is no LDS
// and no barrier, and a wave beyond Q leaves at once.  A rollout is taken in chunks of 64 poses,
// lane l holding pose t0 + l of the chunk: its xy (one coalesced load, issued a chunk ahead of its
// use, so no global load of a pose sits on the chain), then its segment and wrap count.
//   chain   for each pose of the chunk in turn (the wave in step): the pose's xy is read from its
//           lane, the 64 lanes stride over the candidates of hzn_range, each keeps its least
//           (key, index), the xor butterfly folds them (hzn_locate's, without the LDS step) and
//           the winner, made scalar, is the next pose's hint; lane t keeps seg_t and c_t.
//   poses   every lane computes its own pose's values (hzn_foot on its segment gives the winner's
//           D again, bit for bit) and stores them, consecutive lanes to consecutive elements.
//   sums    the lanes' terms are read in ascending t and added in that order, by all lanes alike;
//           lane 0 writes the per-rollout values after the last chunk.
// No atomics: every output element has one writer.
__global__ __launch_bounds__(RLL_THREADS) void rl_rollout_kernel(RllParams p) {
    const TrajParams& q = p.src;
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * RLL_WAVES + (threadIdx.x >> 6);
    if (k >= p.Q) return;
    const int N = q.N, T = p.T;
    const int S = q.closed ? N : N - 1;
    const int r = p.row ? p.row[k] : 0, b = hzn_instance(q, r);
    const bool has_row = b >= 0 && b < q.B && S >= 1;      // else: no row, or a row without a segment
    const size_t off = has_row ? (size_t)b * (size_t)N : 0, boff = has_row ? (size_t)r * (size_t)N : 0;
    const double *x = q.x + off, *y = q.y + off, *vr = q.v + off;
    const double *lo = p.lo + boff, *hi = p.hi + boff;
    const double h = has_row ? hzn_step(q, b) : 0.0;
    const size_t base = (size_t)k * (size_t)T;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    bool alive = has_row;
    int count = has_row ? T : 0;
    int g = p.hint ? p.hint[k] : -1, prev = -1, cw = 0, first_out = T;
    double E = 0.0, O = 0.0, V = 0.0, e_max = 0.0, m_min = INFINITY, s_first = nan, s_last = nan;
    double nx = 0.0, ny = 0.0;                               // the next chunk's pose of this lane
    if (lane < T) {
        nx = p.xy[2 * (base + lane)];
        ny = p.xy[2 * (base + lane) + 1];
    }
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int n = min(64, T - t0), t = t0 + lane;
        const double px = nx, py = ny;
        if (t + 64 < T) {
            nx = p.xy[2 * (base + t + 64)];
            ny = p.xy[2 * (base + t + 64) + 1];
        }
        int myseg = -1, myc = 0, located = 0;
        if (alive) {
            for (int tt = 0; tt < n; ++tt) {
                const double qx = lane_f64(px, tt), qy = lane_f64(py, tt);
                const HznRange rg = hzn_range(q.closed, S, g, t0 + tt == 0 ? p.window0 : p.window);
                uint64_t bk = HZN_KEY_NONE;
                uint32_t bi = HZN_IDX_NONE;
                for (int c = lane; c < rg.C; c += 64) {
                    int i = rg.lo + c;
                    if (i < 0) i += S;
                    else if (i >= S) i -= S;
                    const int j = i + 1 < N ? i + 1 : 0;
                    const double D = foot(x[i], y[i], x[j], y[j], qx, qy).D;
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
                // every lane holds the winner: as scalars, so the chain's control flow is the wave's
                const uint32_t wi = (uint32_t)__builtin_amdgcn_readfirstlane((int)bi);
                const uint32_t wk = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bk >> 32));
                if (wk >= (uint32_t)(HZN_KEY_NAN >> 32) || wi >= (uint32_t)S) {   // a NaN winner, or no candidate at all
                    alive = false;
                    count = t0 + tt;
                    break;
                }
                const int seg = (int)wi;
                if (q.closed && prev >= 0) {
                    const int d = seg - prev;
                    if (2 * d < -S) ++cw;
                    else if (2 * d > S) --cw;
                }
                prev = g = seg;
                if (lane == tt) {
                    myseg = seg;
                    myc = cw;
                }
                ++located;
            }
        }
        // this lane's pose
        const bool loc = lane < located;
        double u = nan, e = nan, d2 = nan, s = nan, m = nan, vf = nan, te = 0.0, to = 0.0, tv = 0.0, ae = 0.0;
        if (loc) {
            const Foot f = hzn_foot(x, y, N, myseg, px, py);
            const double root = sqrt(f.D);
            const int j = myseg + 1 < N ? myseg + 1 : 0;
            u = f.u;
            d2 = f.D;
            e = (f.dx * f.wy - f.dy * f.wx) < 0.0 ? -root : root;        // hzn_store_loc's sign
            s = (((double)myc * (double)S + (double)myseg) + u) * h;      // hzn_columns' form
            const double lo_t = smax(lo[myseg], lo[j]), hi_t = smin(hi[myseg], hi[j]);
            m = smin(hi_t - e, e - lo_t);
            const double vi = vr[myseg];
            vf = vi + u * (vr[j] - vi);
            te = e * e;
            to = m < 0.0 ? m * m : 0.0;
            if (p.v) {
                const double dv = p.v[base + t] - vf;
                tv = dv * dv;
            }
            ae = fabs(e);
        }
        if (lane < n) {
            p.seg[base + t] = loc ? myseg : -1;
            const double val[RLL_POSE_F64] = {u, e, d2, s, m, vf};
#pragma unroll
            for (int c = 0; c < RLL_POSE_F64; ++c) p.pose[c][base + t] = val[c];
        }
        // the sums, in ascending t
        for (int tt = 0; tt < located; ++tt) {
            E = E + lane_f64(te, tt);
            O = O + lane_f64(to, tt);
            V = V + lane_f64(tv, tt);
            e_max = smax(e_max, lane_f64(ae, tt));
            m_min = smin(m_min, lane_f64(m, tt));
        }
        const unsigned long long out = __ballot(loc && m < 0.0);
        if (out && first_out == T) first_out = t0 + __builtin_ctzll(out);
        if (located > 0) {
            if (t0 == 0) s_first = lane_f64(s, 0);
            s_last = lane_f64(s, located - 1);
        }
    }
    if (lane == 0) {
        const bool valid = count == T;
        double progress = nan, cost = nan;
        if (valid) {
            progress = s_last - s_first;
            cost = ((p.w_e * E + p.w_out * O) + p.w_v * V) - p.w_prog * progress;
            if (p.hard_bounds && first_out < T) cost = INFINITY;
        }
        p.head[0][k] = progress;
        p.head[1][k] = e_max;
        p.head[2][k] = m_min;
        p.head[3][k] = cost;
        p.ihead[0][k] = count;
        p.ihead[1][k] = valid ? 1 : 0;
        p.ihead[2][k] = first_out;
    }
}

hipError_t launch_rollouts(const RllParams& p, hipStream_t st) {
    if (p.Q <= 0 || p.T <= 0) return hipSuccess;
    hipLaunchKernelGGL(rl_rollout_kernel, dim3((unsigned)((p.Q + RLL_WAVES - 1) / RLL_WAVES)), dim3(RLL_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace rl
