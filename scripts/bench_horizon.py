"""Look-ahead horizons from poses: the horizon stage against the host route, on the GPU, in one
process.

Set-up: workload C2's plan (competition_map1, N=2000, B=1024 seeds, 14 outer iterations), run
once, the winner selected by lap, its trajectory stage resident (dt = 0.05 s, M_cap = 1024).
Then horizons of M_cap = 64 ticks, 0.05 s apart.  The variants are interleaved by
stage_bench.interleave (>= 20 calls each after warm-up) and reported as medians with min-max:

  dev_q1_hint     Plan.horizon + fetch_horizon of one pose with a hint and a window of 16 segments
  dev_q1_nohint   the same pose without a hint (all N segments)
  dev_q1024       1024 poses jittered around the raceline, without hints
  host_*          raceline.horizon_host of the same poses on rows and stamps that are already on
                  the host: the route a caller had before this stage, after its one download
  host_download   that download: fetch_selected, fetch_lap (min-curvature: heading, curvature, v
                  and ax of every instance, the lap stage has no narrower fetch) and
                  fetch_trajectory.  Needed once per run, not once per pose.

The host clock around a device variant ends after fetch_horizon, which synchronises;
rl_plan_kernel_ms(8) is the stage's device time (upload excluded) of the same call.

  python scripts/bench_horizon.py [--mode mintime] [--calls 20] [--out profiles/horizon_c2.json]
"""
import numpy as np

import stage_bench as sb
from stage_bench import raceline

QUERIES = ("q1_hint", "q1_nohint", "q1024")


def variants(a):
    return [f"dev_{q}" for q in QUERIES] + [f"host_{q}" for q in QUERIES] + ["host_download"]


def main():
    ap = sb.parser("bench_horizon", mode="mincurv", cap=64, queries=True)
    ap.add_argument("--window", type=int, default=16)
    a = sb.parse(ap, variants)
    c2 = sb.c2_setup(a, a.mode)
    pl, prob, N, (rows, h, stamps) = c2.pl, c2.prob, c2.prob.N, c2[3:6]
    g = N // 3
    one, many = sb.jittered_poses(rows[0], rows[1], prob, a.queries)
    hint = np.array([g], dtype=np.int32)
    queries = dict(zip(QUERIES, (dict(poses=one, seg_hint=hint, window=a.window), dict(poses=one), dict(poses=many))))

    def call(v):
        if v == "host_download":
            return sb.download(pl, prob, a.mode)
        if v.startswith("dev_"):
            pl.horizon(dt=a.dt, m_cap=a.cap, **queries[v[4:]])
            return pl.fetch_horizon()
        return raceline.horizon_host(*rows, h, prob.closed, dt=a.dt, m_cap=a.cap, stamps=stamps, **queries[v[5:]])

    t, res = sb.interleave(pl, variants(a), call, lambda v: 8 if v.startswith("dev_") else None, a.calls, a.warmup)
    pl.close()
    rec = {**sb.header(a, N, a.mode), "window": a.window, "Q_many": a.queries, "calls_per_variant": a.calls,
           "warmup_calls": a.warmup, **sb.blocks(t)}
    for q in queries:
        rec[f"dev_over_host_{q}"] = round(rec[f"dev_{q}"]["host_ms"]["median"] / rec[f"host_{q}"]["host_ms"]["median"], 6)
        rec[f"bit_equal_{q}"] = bool(sb.same_answer(res[f"dev_{q}"], res[f"host_{q}"]))
    rec["located"] = {"seg": int(res["dev_q1_hint"].seg[0]), "hint": g, "e_m": float(res["dev_q1_hint"].e[0]),
                      "t0_s": float(res["dev_q1_hint"].t0[0]), "T_s": float(stamps[0, N if prob.closed else N - 1])}
    sb.write(a, "variants interleaved call by call in one process in a rotating order, warm-up calls dropped; host clock around "
                "Plan.horizon + fetch_horizon (which synchronises) and around horizon_host on rows and stamps already "
                "on the host; rl_plan_kernel_ms(8) of the same call; host_download is the one-off download the host "
                "route needs after a run", [rec])
    sb.summarise(rec)


if __name__ == "__main__":
    main()
