"""Sampled trajectories scored against the plan: the rollout stage against the route a caller had
before it (the horizon stage, one workgroup per pose, then a reduction in NumPy), on the GPU, in
one process.

Set-up: workload C2's plan (competition_map1, N=2000, B=1024 seeds, 14 outer iterations), run
once, the winner selected by lap, its trajectory and bounds stages resident.  The rollouts step one
sample per pose along the winner from random samples, jittered by 0.3 m, each with the row's own
speed plus noise.  The variants are interleaved call by call, in stage_bench.rounds' rotating
order (>= 20 calls each after warm-up, the warm-up calls dropped), and reported as medians with
min-max:

  rll_q1024_t64      Plan.rollouts (window 8, hints at the first poses) + fetch_rollouts (the
                     per-rollout values and order; the per-pose arrays stay on the device)
  hzn_q65536         the same 65 536 poses through Plan.horizon (M_cap = 1, the chained hints taken
                     from a prior run, the same window) + fetch_horizon, then the reduction of
                     rollouts_host's sums in NumPy (reduce_host below)
  rll_q1_t64, rll_q16384_t64, rll_q1024_t512    the scaling in Q and T

The host clock around a variant ends after the fetch, which synchronises (and, for hzn_q65536,
after the reduction); rl_plan_kernel_ms(16) / (8) is the stage's device time of the same call.
chain_us_per_pose is the serial chain's cost per pose: the difference of the T = 512 and T = 64
device times at Q = 1 024 over the 448 poses between them (all 1 024 waves are resident at once, so
the difference is the chain's length, not the machine's width).  No target is set.

  python scripts/bench_rollouts.py [--calls 20] [--out profiles/rollouts_c2.json]
"""
import numpy as np

import stage_bench as sb
from stage_bench import raceline

SHAPES = {"rll_q1024_t64": (1024, 64), "rll_q1_t64": (1, 64), "rll_q16384_t64": (16384, 64), "rll_q1024_t512": (1024, 512)}
WINDOW = 8
WEIGHTS = (1.0, 100.0, 0.1, 1.0)


def variants(a):
    return ["rll_q1024_t64", "hzn_q65536", "rll_q1_t64", "rll_q16384_t64", "rll_q1024_t512"]


def make(rows, prob, Q, T):
    """(xy [Q, T, 2], speeds [Q, T], hint [Q]) along row 0."""
    rng = np.random.default_rng(1)
    N = prob.N
    S = N if prob.closed else N - 1
    start = rng.integers(0, N if prob.closed else max(N - T, 1), size=Q)
    at = start[:, None] + np.arange(T)[None]
    at = at % N if prob.closed else np.minimum(at, N - 1)
    xy = np.stack([rows[0][0, at], rows[1][0, at]], axis=2) + rng.normal(size=(Q, T, 2)) * 0.3
    return np.ascontiguousarray(xy), rows[4][0, at] + rng.normal(size=(Q, T)), np.minimum(start, S - 1).astype(np.int32)


def reduce_host(hz, Q, T, rows, h, bnd, prob, speeds):
    """What a caller of the horizon route computes on the host: rollouts_host's per-rollout values
    from the located poses (vectorised over the rollouts; the sums by np.cumsum, which adds
    serially in t)."""
    N = prob.N
    S = N if prob.closed else N - 1
    seg, u, e = hz.seg.reshape(Q, T), hz.u.reshape(Q, T), hz.e.reshape(Q, T)
    j = (seg + 1) % N
    lo, hi, V = bnd.lo[0], bnd.hi[0], rows[4][0]
    d = np.diff(seg, axis=1)
    c = np.zeros((Q, T))
    if prob.closed:
        c[:, 1:] = np.cumsum(np.where(2 * d < -S, 1.0, np.where(2 * d > S, -1.0, 0.0)), axis=1)
    s = ((c * np.float64(S) + seg.astype(np.float64)) + u) * h
    lo_t, hi_t = np.where(lo[seg] < lo[j], lo[j], lo[seg]), np.where(hi[j] < hi[seg], hi[j], hi[seg])
    m1, m2 = hi_t - e, e - lo_t
    m = np.where(m2 < m1, m2, m1)
    vref = V[seg] + u * (V[j] - V[seg])
    E = np.cumsum(e * e, axis=1)[:, -1]
    Oo = np.cumsum(np.where(m < 0.0, m * m, 0.0), axis=1)[:, -1]
    dv = speeds - vref
    Vv = np.cumsum(dv * dv, axis=1)[:, -1]
    prog = s[:, -1] - s[:, 0]
    w_e, w_out, w_v, w_prog = WEIGHTS
    return ((w_e * E + w_out * Oo) + w_v * Vv) - w_prog * prog


def main():
    ap = sb.parser("bench_rollouts", mode="mintime", cap=1)
    a = sb.parse(ap, variants)
    c2 = sb.c2_setup(a, a.mode, bounds=True)
    pl, prob, rows, h, bnd = c2.pl, c2.prob, c2.rows, c2.h, c2.bnd
    data = {v: make(rows, prob, *qt) for v, qt in SHAPES.items()}
    xy, speeds, hint0 = data["rll_q1024_t64"]
    Q, T = xy.shape[:2]
    # the chained hints of the horizon route, from a prior run of the stage
    pl.rollouts(xy, v=speeds, seg_hint=hint0, window0=WINDOW, window=WINDOW, weights=WEIGHTS)
    prior = pl.fetch_rollouts(poses=True)
    assert np.all(prior.valid == 1)
    chained = np.ascontiguousarray(np.concatenate([hint0[:, None], prior.seg[:, :-1]], axis=1).reshape(-1))
    flat = np.ascontiguousarray(xy.reshape(Q * T, 2))

    def call(v):
        if v == "hzn_q65536":
            pl.horizon(flat, seg_hint=chained, window=WINDOW, dt=a.dt, m_cap=1)
            return reduce_host(pl.fetch_horizon(), Q, T, rows, h, bnd, prob, speeds)
        P, V, g = data[v]
        pl.rollouts(P, v=V, seg_hint=g, window0=WINDOW, window=WINDOW, weights=WEIGHTS)
        return pl.fetch_rollouts()

    t, res = sb.interleave(pl, variants(a), call, lambda v: 8 if v == "hzn_q65536" else 16, a.calls, a.warmup)
    rec = {**sb.header(a, prob.N, a.mode), "window": WINDOW, "weights": list(WEIGHTS), "calls_per_variant": a.calls,
           "warmup_calls": a.warmup}
    rec["bit_equal_cost"] = bool(np.array_equal(res["rll_q1024_t64"].cost.view(np.uint64), res["hzn_q65536"].view(np.uint64)))
    pl.close()
    rec.update(sb.blocks(t))
    med = sb.medians(rec)
    for v, (q, tt) in SHAPES.items():
        rec[f"kernel_ns_per_pose_{v}"] = round(med(v, "kernel_ms") * 1e6 / (q * tt), 3)
    rec["kernel_ns_per_pose_hzn_q65536"] = round(med("hzn_q65536", "kernel_ms") * 1e6 / (Q * T), 3)
    rec["rll_over_hzn_kernel"] = round(med("rll_q1024_t64", "kernel_ms") / med("hzn_q65536", "kernel_ms"), 4)
    rec["rll_over_hzn_call"] = round(med("rll_q1024_t64", "host_ms") / med("hzn_q65536", "host_ms"), 4)
    rec["chain_us_per_pose"] = round((med("rll_q1024_t512", "kernel_ms") - med("rll_q1024_t64", "kernel_ms")) * 1e3 / 448.0, 4)
    sb.write(a, "variants interleaved call by call in one process in a rotating order, warm-up calls dropped; host clock around "
                "Plan.rollouts + fetch_rollouts (which synchronises) and around Plan.horizon + fetch_horizon + the NumPy "
                "reduction; rl_plan_kernel_ms(16) / (8) of the same call", [rec])
    sb.summarise(rec)


if __name__ == "__main__":
    main()
