"""Braking to a target speed at a sample: the stop stage against the rejoin stage and the host
route, on the GPU, in one process.

Set-up: workload C2's plan (competition_map1, N=2000, B=1024 seeds, 14 outer iterations), run
once, the winner selected by lap, its trajectory stage resident (dt = 0.05 s, M_cap = 1024).
Then M_cap = 64 ticks, 0.05 s apart, K_cap = 1024 nodes, every pose at the raceline's own speed,
the target speed 0.  The variants are interleaved by stage_bench.interleave (>= 20 calls each
after warm-up) and reported as medians with min-max:

  stp_q1_k64, stp_q1_k1024        Plan.stop + fetch_stop of one pose, the target 64 / 1024 samples
                                  ahead of its segment (1024: the full serial chain, twice)
  stp_q1024_k64, stp_q1024_k1024  1024 poses jittered around the raceline, the same targets
  rjn_q1, rjn_q1024               Plan.rejoin + fetch_rejoin of the same poses from standstill: one
                                  serial chain where the stop stage has two
  host_*                          raceline.stop_host of the same queries on rows and stamps that
                                  are already on the host

The host clock around a device variant ends after the fetch, which synchronises;
rl_plan_kernel_ms(10) (9 for the rejoin stage) is the stage's device time (upload excluded) of the
same call.  The figure of interest is the device time per node of the two serial chains against
the rejoin stage's per marched node; it is no roofline fraction.

  python scripts/bench_stop.py [--mode mintime] [--calls 20] [--out profiles/stop_c2.json]
"""
import numpy as np

import stage_bench as sb
from stage_bench import abi, raceline

K_CAP = abi.RL_RJN_MAX_NODES
POSES = ("q1", "q1024")
STP = {f"{q}_k{k}": (q, k) for q in POSES for k in (64, K_CAP)}


def variants(a):
    return [f"stp_{s}" for s in STP] + [f"rjn_{q}" for q in POSES] + [f"host_{s}" for s in STP]


def main():
    a = sb.parse(sb.parser("bench_stop", mode="mincurv", cap=64, queries=True), variants)
    c2 = sb.c2_setup(a, a.mode)
    pl, prob, cfg, rows, h, stamps = c2[:6]
    poses = dict(zip(POSES, sb.jittered_poses(rows[0], rows[1], prob, a.queries, K_CAP)))
    own, seg = {}, {}
    for q, P in poses.items():
        own[q], seg[q] = sb.own_speed(c2, P, a.dt)
    stp = {s: (q, sb.target(seg[q], k, prob)) for s, (q, k) in STP.items()}

    def call(v):
        if v.startswith("stp_"):
            q, J = stp[v[4:]]
            pl.stop(poses[q], own[q], cfg, J, 0.0, dt=a.dt, m_cap=a.cap, k_cap=K_CAP)
            return pl.fetch_stop(nodes=False)
        if v.startswith("rjn_"):
            pl.rejoin(poses[v[4:]], 0.0, cfg, dt=a.dt, m_cap=a.cap, k_cap=K_CAP)
            return pl.fetch_rejoin(nodes=False)
        q, J = stp[v[5:]]
        return raceline.stop_host(*rows, h, prob.closed, poses[q], own[q], cfg, J, 0.0, dt=a.dt, m_cap=a.cap, k_cap=K_CAP,
                                  stamps=stamps)

    t, res = sb.interleave(pl, variants(a), call, lambda v: {"stp_": 10, "rjn_": 9}.get(v[:4]), a.calls, a.warmup)
    pl.close()
    rec = {**sb.header(a, prob.N, a.mode), "K_cap": K_CAP, "Q_many": a.queries, "calls_per_variant": a.calls,
           "warmup_calls": a.warmup, "h_m": float(np.ravel(h)[0]), **sb.blocks(t)}
    for q in poses:
        r = res[f"rjn_{q}"]
        ke = np.array([r.node_end(i) for i in range(len(r.count))])
        rec[f"rjn_nodes_marched_{q}"] = {"median": float(np.median(ke)), "min": int(ke.min()), "max": int(ke.max())}
        rec[f"rjn_us_per_node_of_longest_march_{q}"] = round(rec[f"rjn_{q}"]["kernel_ms"]["median"] * 1e3 / max(int(ke.max()), 1), 4)
    for s in stp:
        want, got = res[f"host_{s}"], res[f"stp_{s}"]
        ks = want.stop_node
        rec[f"stop_node_{s}"] = {"min": int(ks.min()), "max": int(ks.max()), "reachable": int(want.reachable.sum()), "of": int(len(ks))}
        rec[f"bit_equal_{s}"] = bool(sb.same_answer(got, want, mask="stop_node"))
        # two serial chains of K_s nodes each: the device time of the whole stage per node of one chain
        rec[f"us_per_node_{s}"] = round(rec[f"stp_{s}"]["kernel_ms"]["median"] * 1e3 / max(int(ks.max()), 1), 4)
        rec[f"dev_over_host_{s}"] = round(rec[f"stp_{s}"]["host_ms"]["median"] / rec[f"host_{s}"]["host_ms"]["median"], 6)
    sb.write(a, "variants interleaved call by call in one process in a rotating order, warm-up calls dropped; host clock around "
                "Plan.stop + fetch_stop / Plan.rejoin + fetch_rejoin (which synchronise) and around stop_host on rows and "
                "stamps already on the host; rl_plan_kernel_ms(10) / (9) of the same call", [rec])
    sb.summarise(rec)


if __name__ == "__main__":
    main()
