"""The look-ahead speed profile under other limits: the retime stage against the stop stage and the
host route, on the GPU, in one process.

Set-up: workload C2's plan (competition_map1, N=2000, B=1024 seeds, 14 outer iterations), run
once, the winner selected by lap, its trajectory stage resident (dt = 0.05 s, M_cap = 1024).
Then M_cap = 64 ticks, 0.05 s apart, every pose at the raceline's own speed, the query's cfg a wet
one (mu = 0.8, the lateral limit lowered with it).  The variants are interleaved by
stage_bench.interleave (>= 20 calls each after warm-up) and reported as medians with min-max:

  rtm_q1_k64, rtm_q1_k1024        Plan.retime + fetch_retime of one pose over K_cap = 64 / 1024 nodes
                                  (1024: the full serial chains, one backward and one forward)
  rtm_q1024_k64, rtm_q1024_k1024  1024 poses jittered around the raceline, the same K_cap
  stp_q1_k1024, stp_q1024_k1024   Plan.stop + fetch_stop of the same poses to a target 1024 samples
                                  ahead: the stop stage's two chains, in the same process
  host_*                          raceline.retime_host of the same queries on rows and stamps that
                                  are already on the host; the 1024-pose ones take seconds each and
                                  are called --host-calls times only ("n" says how often)

The host clock around a device variant ends after the fetch, which synchronises;
rl_plan_kernel_ms(13) (10 for the stop stage) is the stage's device time (upload excluded) of the
same call.  The figure of interest is the device time per node and pass (two serial passes over K
nodes, and the parallel ceiling pass) against the stop stage's; it is no roofline fraction.

  python scripts/bench_retime.py [--mode mintime] [--calls 20] [--out profiles/retime_c2.json]
"""
import numpy as np

import stage_bench as sb
from stage_bench import abi, raceline

K_CAP = abi.RL_RJN_MAX_NODES
POSES = ("q1", "q1024")
RTM = {f"{q}_k{k}": (q, k) for q in POSES for k in (64, K_CAP)}
STP = [f"{q}_k{K_CAP}" for q in POSES]


def variants(a):
    return [f"rtm_{s}" for s in RTM] + [f"stp_{s}" for s in STP] + [f"host_{s}" for s in RTM]


def main():
    ap = sb.parser("bench_retime", mode="mincurv", cap=64, queries=True)
    ap.add_argument("--host-calls", type=int, default=1)
    a = sb.parse(ap, variants)
    c2 = sb.c2_setup(a, a.mode)
    pl, prob, cfg, rows, h, stamps = c2[:6]
    wet = sb.wet_cfg(cfg)
    poses = dict(zip(POSES, sb.jittered_poses(rows[0], rows[1], prob, a.queries, K_CAP)))
    own, stp = {}, {}
    for q, P in poses.items():
        own[q], seg = sb.own_speed(c2, P, a.dt)
        stp[f"{q}_k{K_CAP}"] = (q, sb.target(seg, K_CAP, prob))

    def call(v):
        if v.startswith("rtm_"):
            q, k = RTM[v[4:]]
            pl.retime(poses[q], own[q], wet, dt=a.dt, m_cap=a.cap, k_cap=k)
            return pl.fetch_retime(nodes=False)
        if v.startswith("stp_"):
            q, J = stp[v[4:]]
            pl.stop(poses[q], own[q], wet, J, 0.0, dt=a.dt, m_cap=a.cap, k_cap=K_CAP)
            return pl.fetch_stop(nodes=False)
        q, k = RTM[v[5:]]
        return raceline.retime_host(*rows, h, prob.closed, poses[q], own[q], wet, dt=a.dt, m_cap=a.cap, k_cap=k, stamps=stamps)

    t, res = sb.interleave(pl, variants(a), call, lambda v: {"rtm_": 13, "stp_": 10}.get(v[:4]), a.calls, a.warmup,
                           skip=sb.slow_host(a))
    pl.close()
    rec = {**sb.header(a, prob.N, a.mode), "K_cap_max": K_CAP, "Q_many": a.queries, "calls_per_variant": a.calls,
           "host_calls_q1024": a.host_calls, "warmup_calls": a.warmup, "h_m": float(np.ravel(h)[0]),
           "query_cfg": "mu = 0.8, a_lat_max = min(a_lat_max, a_total_max)", **sb.blocks(t)}
    for s in stp:
        ks = res[f"stp_{s}"].stop_node
        # two serial chains of K_s nodes each: the device time of the whole stage per node and pass
        rec[f"stp_us_per_node_and_pass_{s}"] = round(rec[f"stp_{s}"]["kernel_ms"]["median"] * 1e3 / (2 * max(int(ks.max()), 1)), 4)
    for s in RTM:
        want, got = res[f"host_{s}"], res[f"rtm_{s}"]
        ke = want.end_node
        rec[f"end_node_{s}"] = {"min": int(ke.min()), "max": int(ke.max()), "feasible": int(want.feasible.sum()),
                                "bind": int(np.count_nonzero(want.bind_node >= 0)), "of": int(len(ke))}
        rec[f"bit_equal_{s}"] = bool(sb.same_answer(got, want, mask="end_node"))
        # two serial passes over K nodes (the parallel ceiling pass beside them): the device time of
        # the whole stage per node of one pass, and per node and pass
        rec[f"us_per_node_{s}"] = round(rec[f"rtm_{s}"]["kernel_ms"]["median"] * 1e3 / max(int(ke.max()), 1), 4)
        rec[f"us_per_node_and_pass_{s}"] = round(rec[f"us_per_node_{s}"] / 2.0, 4)
        rec[f"dev_over_host_{s}"] = round(rec[f"rtm_{s}"]["host_ms"]["median"] / rec[f"host_{s}"]["host_ms"]["median"], 6)
    sb.write(a, "variants interleaved call by call in one process in a rotating order, warm-up calls dropped; host clock around "
                "Plan.retime + fetch_retime / Plan.stop + fetch_stop (which synchronise) and around retime_host on rows and "
                "stamps already on the host (the 1024-pose host variants host_calls_q1024 times only); "
                "rl_plan_kernel_ms(13) / (10) of the same call", [rec])
    sb.summarise(rec)


if __name__ == "__main__":
    main()
