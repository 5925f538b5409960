// rl_select.hip — the stage after the optimiser: score every instance of a
// batch, rank the instances of each group, and copy the winners' rows into compact buffers,
// so a multi-start caller downloads G*k rows instead of B.  Three small gfx950 kernels on the
// run stream; the winners' indices never leave device memory between them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_select.h"

namespace rl {

// ---------------------------------------------------------------------------- score
// One workgroup of SCORE_T lanes per instance.  The summation order is fixed by N alone:
// lane t adds kappa[t]^2, kappa[t + SCORE_T]^2, ... in that order (coalesced loads), each
// wave folds its 64 partial sums with the tree lane l += lane l + off (off = 32 .. 1), and
// lane 0 adds the SCORE_T / 64 wave sums in wave order.  No atomics, so the bits of score[b]
// depend on nothing but the kappa row, N and h.
constexpr int SCORE_T = 256;

__global__ __launch_bounds__(SCORE_T) void rl_score_kernel(const double* __restrict__ kappa, int N, double L,
                                                           const double* __restrict__ Ls,
                                                           double* __restrict__ score) {
    __shared__ double part[SCORE_T / 64];
    const int b = blockIdx.x;
    const double* k = kappa + (size_t)b * (size_t)N;
    double s = 0.0;
    for (int i = threadIdx.x; i < N; i += SCORE_T) {
        const double v = k[i];
        s = s + v * v;
    }
    for (int off = 32; off; off >>= 1) s = s + __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = part[0];
        for (int w = 1; w < SCORE_T / 64; ++w) t = t + part[w];
        const double h = (Ls ? Ls[b] : L) / (double)N;
        score[b] = h * t;
    }
}

hipError_t launch_score(const double* kappa, int32_t N, int32_t B, double L, const double* Ls, double* score,
                        hipStream_t st) {
    hipLaunchKernelGGL(rl_score_kernel, dim3((unsigned)B), dim3(SCORE_T), 0, st, kappa, N, L, Ls, score);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------- rank
// The order is ascending in (isnan(score), score, index).  A score becomes an unsigned key
// whose integer order is that order: -0.0 is canonicalised to +0.0, negative values have all
// their bits flipped, the others their sign bit set (the usual order-preserving map of IEEE
// doubles; -inf -> 0x000f..., +inf -> 0xfff0...), and every NaN maps to the largest key, so
// NaNs come last and tie among themselves.  Ties are broken by the index.
__device__ __forceinline__ uint64_t order_key(double s) {
    if (s != s) return ~0ull;
    uint64_t b = (uint64_t)__double_as_longlong(s);
    if (s == 0.0) b = 0;
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

// One workgroup per group, k rounds: round r takes the smallest (key, index) that lies
// strictly after round r-1's winner, so nothing is marked or removed and the group is only
// read.  Each lane walks the group in strides of the workgroup and keeps its best candidate;
// the wave folds the 64 candidates with an xor butterfly (every lane ends with the wave's
// best), the waves meet in LDS (one slot per wave, double-buffered by the round's parity so
// one barrier per round is enough), and every lane reads all slots and so knows the winner.
// Any group size: fewer than 64 instances leave lanes without a candidate (the sentinel, which
// loses every comparison); more than the workgroup are covered by the strides.
constexpr int RANK_MAX_T = 1024;
constexpr uint32_t RANK_NONE = 0xffffffffu;

__device__ __forceinline__ bool pair_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
    return ka < kb || (ka == kb && ia < ib);
}

__global__ __launch_bounds__(RANK_MAX_T) void rl_rank_kernel(const double* __restrict__ score, int group_size, int k,
                                                             int32_t* __restrict__ index,
                                                             double* __restrict__ score_sel) {
    __shared__ uint64_t s_key[2][RANK_MAX_T / 64];
    __shared__ uint32_t s_idx[2][RANK_MAX_T / 64];
    const int g = blockIdx.x;
    const size_t base = (size_t)g * (size_t)group_size;
    const double* sc = score + base;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    // the previous winner; no key is 0 (the smallest, -inf's, is 0x000fffffffffffff), so
    // (0, -1) lies before every instance
    uint64_t pk = 0;
    int64_t pi = -1;
    for (int r = 0; r < k; ++r) {
        uint64_t bk = ~0ull;
        uint32_t bi = RANK_NONE;
        for (int j = threadIdx.x; j < group_size; j += blockDim.x) {
            const uint64_t key = order_key(sc[j]);
            const bool after = key > pk || (key == pk && (int64_t)j > pi);
            if (after && pair_less(key, (uint32_t)j, bk, bi)) {
                bk = key;
                bi = (uint32_t)j;
            }
        }
        for (int off = 32; off; off >>= 1) {
            const uint64_t ok = __shfl_xor(bk, off, 64);
            const uint32_t oi = __shfl_xor(bi, off, 64);
            if (pair_less(ok, oi, bk, bi)) {
                bk = ok;
                bi = oi;
            }
        }
        const int buf = r & 1;
        if (lane == 0) {
            s_key[buf][w] = bk;
            s_idx[buf][w] = bi;
        }
        __syncthreads();
        bk = s_key[buf][0];
        bi = s_idx[buf][0];
        for (int q = 1; q < nw; ++q) {
            const uint64_t ok = s_key[buf][q];
            const uint32_t oi = s_idx[buf][q];
            if (pair_less(ok, oi, bk, bi)) {
                bk = ok;
                bi = oi;
            }
        }
        pk = bk;
        pi = (int64_t)bi;
        if (threadIdx.x == 0) {
            // k <= group_size, so every round finds an instance; the guard keeps a caller's
            // mistake from becoming an out-of-range read
            const bool found = bi < (uint32_t)group_size;
            const size_t o = (size_t)g * (size_t)k + (size_t)r;
            index[o] = found ? (int32_t)(base + bi) : -1;
            if (score_sel) score_sel[o] = found ? sc[bi] : __longlong_as_double(0x7ff8000000000000ll);
        }
    }
}

hipError_t launch_rank(const double* score, int32_t B, int32_t group_size, int32_t k, int32_t* index,
                       double* score_sel, hipStream_t st) {
    const int G = B / group_size;
    const int T = group_size <= 64 ? 64 : group_size <= 4096 ? 256 : RANK_MAX_T;
    hipLaunchKernelGGL(rl_rank_kernel, dim3((unsigned)G), dim3(T), 0, st, score, group_size, k, index, score_sel);
    return hipGetLastError();
}

// --------------------------------------------------------------------------- gather
// Workgroup (row, c): c < RL_SEL_F64 copies row index[row] of f64 column c (coalesced),
// c == RL_SEL_F64 the lap and the counters.  An index outside [0, B) copies nothing.
constexpr int GATHER_T = 256;

__global__ __launch_bounds__(GATHER_T) void rl_gather_kernel(GatherParams g) {
    const int row = blockIdx.x, c = blockIdx.y;
    const int32_t b = g.index[row];
    if ((uint32_t)b >= (uint32_t)g.B) return;
    if (c < RL_SEL_F64) {
        const double* s = g.src[c];
        double* d = g.dst[c];
        if (!s || !d) return;
        s += (size_t)b * (size_t)g.N;
        d += (size_t)row * (size_t)g.N;
        for (int i = threadIdx.x; i < g.N; i += GATHER_T) d[i] = s[i];
        return;
    }
    if (g.lap_src && g.lap_dst && threadIdx.x == 0) g.lap_dst[row] = g.lap_src[b];
    for (int i = threadIdx.x; i < g.mo; i += GATHER_T) {
        if (g.evals_src && g.evals_dst) g.evals_dst[(size_t)row * g.mo + i] = g.evals_src[(size_t)b * g.mo + i];
        if (g.accepts_src && g.accepts_dst) g.accepts_dst[(size_t)row * g.mo + i] = g.accepts_src[(size_t)b * g.mo + i];
    }
    if (g.sweeps_src && g.sweeps_dst)
        for (int i = threadIdx.x; i < g.mo + 1; i += GATHER_T)
            g.sweeps_dst[(size_t)row * (g.mo + 1) + i] = g.sweeps_src[(size_t)b * (g.mo + 1) + i];
}

hipError_t launch_gather(const GatherParams& g, hipStream_t st) {
    hipLaunchKernelGGL(rl_gather_kernel, dim3((unsigned)g.rows, RL_SEL_F64 + 1), dim3(GATHER_T), 0, st, g);
    return hipGetLastError();
}

}  // namespace rl
