"""A path from the car's offset back to the raceline: the recover stage against the retime stage and
the host route, on the GPU, in one process.

Set-up: workload C2's plan (competition_map1, N=2000, B=1024 seeds, 14 outer iterations), run
once, the winner selected by lap, its trajectory stage (dt = 0.05 s, M_cap = 1024) and its bounds
stage resident.  Then M_cap = 64 ticks, 0.05 s apart, every pose at the raceline's own speed, the
plan's cfg, a merge length of 25 m and the car heading 10 degrees left of the raceline.  The
variants are interleaved by stage_bench.interleave (>= 20 calls each after warm-up) and reported
as medians with min-max:

  rcv_q1_k64, rcv_q1_k512         Plan.recover + fetch_recover of one pose over K_cap = 64 / 512 nodes
  rcv_q1024_k64, rcv_q1024_k512   1024 poses jittered around the raceline, the same K_cap
  rtm_*                           Plan.retime + fetch_retime of the same poses, speeds, cfg, K_cap and
                                  M_cap: the same two serial passes without the offset path
  host_*                          raceline.recover_host of the same queries on rows, stamps and bounds
                                  that are already on the host; the 1024-pose ones take seconds each
                                  and are called --host-calls times only ("n" says how often)

The host clock around a device variant ends after the fetch, which synchronises;
rl_plan_kernel_ms(14) (13 for the retime stage) is the stage's device time (upload excluded) of the
same call.  The expectation to confirm or refute: the stage costs the retime stage's serial passes
plus parallel phases that are small beside them; "rcv_minus_rtm_kernel_ms_*" is the difference of
the medians and "rtm_spread_kernel_ms_*" the retime figure's max - min in this file.

  python scripts/bench_recover.py [--calls 20] [--out profiles/recover_c2.json]
"""
import numpy as np

import stage_bench as sb
from stage_bench import abi, raceline

HEADING_TOL = 2.0 ** -49               # atan2_cr on the device, math.atan2 on the host (tests/recover_cases.py)
K_CAP = abi.RL_RCV_MAX_NODES
POSES = ("q1", "q1024")
SHAPES = {f"{q}_k{k}": (q, k) for q in POSES for k in (64, K_CAP)}


def variants(a):
    return [f"{kind}_{s}" for s in SHAPES for kind in ("rcv", "rtm")] + [f"host_{s}" for s in SHAPES]


def main():
    ap = sb.parser("bench_recover", cap=64, queries=True)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--merge-len", type=float, default=25.0)
    a = sb.parse(ap, variants)
    c2 = sb.c2_setup(a, "mintime", bounds=True)
    pl, prob, cfg, rows, h, stamps, bnd = c2
    poses, dirs = (dict(zip(POSES, x)) for x in sb.beside_poses(rows, bnd, prob, a.queries, K_CAP))
    own = {q: sb.own_speed(c2, P, a.dt)[0] for q, P in poses.items()}

    def call(v):
        kind, s = v.split("_", 1)
        q, k = SHAPES[s]
        if kind == "rcv":
            pl.recover(poses[q], own[q], cfg, a.merge_len, dirs[q], dt=a.dt, m_cap=a.cap, k_cap=k)
            return pl.fetch_recover(nodes=False)
        if kind == "rtm":
            pl.retime(poses[q], own[q], cfg, dt=a.dt, m_cap=a.cap, k_cap=k)
            return pl.fetch_retime(nodes=False)
        return raceline.recover_host(*rows, h, prob.closed, bnd.lo, bnd.hi, poses[q], own[q], cfg, a.merge_len, dirs[q],
                                     nx=bnd.nx, ny=bnd.ny, dt=a.dt, m_cap=a.cap, k_cap=k, stamps=stamps)

    t, res = sb.interleave(pl, variants(a), call, lambda v: {"rcv_": 14, "rtm_": 13}.get(v[:4]), a.calls, a.warmup,
                           skip=sb.slow_host(a))
    pl.close()
    rec = {**sb.header(a, prob.N, "mintime"), "K_cap_max": K_CAP, "Q_many": a.queries, "calls_per_variant": a.calls,
           "host_calls_q1024": a.host_calls, "warmup_calls": a.warmup, "h_m": float(h), "merge_len_m": a.merge_len,
           "dir": "the raceline's heading + 10 degrees", "query_cfg": "the plan's", **sb.blocks(t)}
    for s in SHAPES:
        want, got = res[f"host_{s}"], res[f"rcv_{s}"]
        ke = want.end_node
        rec[f"end_node_{s}"] = {"min": int(ke.min()), "max": int(ke.max()), "feasible": int(want.feasible.sum()),
                                "clamped": int(np.count_nonzero(want.clamped > 0)), "merged": int(np.count_nonzero(want.merge_node >= 0)),
                                "offtrack": int(want.offtrack.sum()), "of": int(len(ke))}
        # bit for bit in everything fetched but heading, which is within HEADING_TOL
        rec[f"equal_{s}"] = bool(sb.same_answer(got, want, mask="end_node", heading_tol=HEADING_TOL))
        rk, tk = rec[f"rcv_{s}"]["kernel_ms"], rec[f"rtm_{s}"]["kernel_ms"]
        rec[f"us_per_node_and_pass_{s}"] = round(rk["median"] * 1e3 / (2 * max(int(ke.max()), 1)), 4)
        rec[f"rcv_minus_rtm_kernel_ms_{s}"] = round(rk["median"] - tk["median"], 4)
        rec[f"rtm_spread_kernel_ms_{s}"] = round(tk["max"] - tk["min"], 4)
        rec[f"dev_over_host_{s}"] = round(rec[f"rcv_{s}"]["host_ms"]["median"] / rec[f"host_{s}"]["host_ms"]["median"], 6)
    sb.write(a, "variants interleaved call by call in one process in a rotating order, warm-up calls dropped; host clock around "
                "Plan.recover + fetch_recover / Plan.retime + fetch_retime (which synchronise) and around recover_host on rows, "
                "stamps and bounds already on the host (the 1024-pose host variants host_calls_q1024 times only); "
                "rl_plan_kernel_ms(14) / (13) of the same call", [rec])
    sb.summarise(rec)


if __name__ == "__main__":
    main()
