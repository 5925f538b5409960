"""Reachable speed profiles from the car's speed: the rejoin stage against the horizon stage and
the host route, on the GPU, in one process.

Set-up: workload C2's plan (competition_map1, N=2000, B=1024 seeds, 14 outer iterations), run
once, the winner selected by lap, its trajectory stage resident (dt = 0.05 s, M_cap = 1024).
Then M_cap = 64 ticks, 0.05 s apart, K_cap = 1024 march nodes.  The variants are interleaved by
stage_bench.interleave (>= 20 calls each after warm-up) and reported as medians with min-max:

  rjn_q1_stand    Plan.rejoin + fetch_rejoin of one pose from standstill
  rjn_q1_09       the same pose at 0.9 x the raceline's own speed there
  rjn_q1024_*     1024 poses jittered around the raceline, from standstill / at 0.9 x
  hzn_q1, hzn_q1024   Plan.horizon + fetch_horizon of the same poses: what the march adds
  host_*          raceline.rejoin_host of the same queries on rows and stamps that are already on
                  the host: the route a caller had before this stage, after its one download
  host_download   that download (fetch_selected, fetch_lap for min-curvature, fetch_trajectory).
                  Needed once per run, not once per pose.

The host clock around a device variant ends after the fetch, which synchronises;
rl_plan_kernel_ms(9) (8 for the horizon) is the stage's device time (upload excluded) of the same
call.  nodes_marched is K_end of each query: the length of the serial chain lane 0 walks.

  python scripts/bench_rejoin.py [--mode mintime] [--calls 20] [--out profiles/rejoin_c2.json]
"""
import numpy as np

import stage_bench as sb
from stage_bench import abi, raceline

POSES = ("q1", "q1024")
SPEEDS = [f"{q}_stand" for q in POSES] + [f"{q}_09" for q in POSES]


def variants(a):
    return [f"rjn_{s}" for s in SPEEDS] + [f"hzn_{q}" for q in POSES] + [f"host_{s}" for s in SPEEDS] + ["host_download"]


def main():
    ap = sb.parser("bench_rejoin", mode="mincurv", cap=64, queries=True)
    ap.add_argument("--nodes", type=int, default=abi.RL_RJN_MAX_NODES)
    a = sb.parse(ap, variants)
    c2 = sb.c2_setup(a, a.mode)
    pl, prob, cfg, rows, h, stamps = c2[:6]
    poses = dict(zip(POSES, sb.jittered_poses(rows[0], rows[1], prob, a.queries)))
    speed = {f"{q}_stand": np.zeros(len(P)) for q, P in poses.items()}
    speed.update({f"{q}_09": 0.9 * sb.own_speed(c2, P, a.dt)[0] for q, P in poses.items()})

    def call(v):
        if v == "host_download":
            return sb.download(pl, prob, a.mode)
        if v.startswith("rjn_"):
            pl.rejoin(poses[v[4:].split("_")[0]], speed[v[4:]], cfg, dt=a.dt, m_cap=a.cap, k_cap=a.nodes)
            return pl.fetch_rejoin(nodes=False)
        if v.startswith("hzn_"):
            pl.horizon(poses[v[4:]], dt=a.dt, m_cap=a.cap)
            return pl.fetch_horizon()
        return raceline.rejoin_host(*rows, h, prob.closed, poses[v[5:].split("_")[0]], speed[v[5:]], cfg, dt=a.dt,
                                    m_cap=a.cap, k_cap=a.nodes, stamps=stamps)

    t, res = sb.interleave(pl, variants(a), call, lambda v: {"rjn_": 9, "hzn_": 8}.get(v[:4]), a.calls, a.warmup)
    pl.close()
    rec = {**sb.header(a, prob.N, a.mode), "K_cap": a.nodes, "Q_many": a.queries, "calls_per_variant": a.calls,
           "warmup_calls": a.warmup, "h_m": float(np.ravel(h)[0]), **sb.blocks(t)}
    for s in speed:
        want, got = res[f"host_{s}"], res[f"rjn_{s}"]
        ke = np.array([want.node_end(q) for q in range(len(want.count))])
        rec[f"nodes_marched_{s}"] = {"median": float(np.median(ke)), "min": int(ke.min()), "max": int(ke.max()),
                                     "merged": int(np.count_nonzero(want.merge_node >= 0)), "of": int(len(ke))}
        rec[f"bit_equal_{s}"] = bool(sb.same_answer(got, want))
        q = s.split("_")[0]
        rec[f"kernel_over_horizon_{s}"] = round(rec[f"rjn_{s}"]["kernel_ms"]["median"] / rec[f"hzn_{q}"]["kernel_ms"]["median"], 3)
        rec[f"dev_over_host_{s}"] = round(rec[f"rjn_{s}"]["host_ms"]["median"] / rec[f"host_{s}"]["host_ms"]["median"], 6)
    # the march alone: the device time the stage adds to the horizon's, per node of the longest chain
    for s in speed:
        q = s.split("_")[0]
        extra_us = (rec[f"rjn_{s}"]["kernel_ms"]["median"] - rec[f"hzn_{q}"]["kernel_ms"]["median"]) * 1e3
        rec[f"extra_us_per_node_of_longest_march_{s}"] = round(extra_us / max(rec[f"nodes_marched_{s}"]["max"], 1), 4)
    w = res["host_q1_stand"]
    rec["standing_start"] = {"merge_node": int(w.merge_node[0]), "t_merge_s": float(w.t_merge[0]), "t_loss_s": float(w.t_loss[0])}
    sb.write(a, "variants interleaved call by call in one process in a rotating order, warm-up calls dropped; host clock around "
                "Plan.rejoin + fetch_rejoin / Plan.horizon + fetch_horizon (which synchronise) and around rejoin_host on rows "
                "and stamps already on the host; rl_plan_kernel_ms(9) / (8) of the same call; host_download is the one-off "
                "download the host route needs after a run", [rec])
    sb.summarise(rec)


if __name__ == "__main__":
    main()
