"""Several merge lengths per pose: the fan stage against the route it replaces (the recover stage
with Q*C queries and a pick on the host) and against one recover stage of Q queries, on the GPU,
in one process.

Set-up: bench_recover.py's: workload C2's plan (competition_map1, N=2000, B=1024 seeds, 14 outer
iterations), run once, the winner selected by lap, its trajectory stage (dt = 0.05 s, M_cap = 1024)
and its bounds stage resident; M_cap = 64 ticks, 0.05 s apart, every pose at the raceline's own
speed, the plan's cfg, the car heading 10 degrees left of the raceline; one pose 0.3 m beside the
line and 1024 poses jittered around it.  The C merge lengths are spaced geometrically from 4 m to
120 m.  The variants are interleaved by stage_bench.interleave (>= 20 calls each after warm-up)
and reported as medians with min-max:

  fan_q*_c*_k*     Plan.recover_fan + fetch_recover_fan(nodes=False): Q poses, C lengths, K_cap nodes
  qc_q*_c*_k*      the existing route: Plan.recover with Q*C queries (every pose C times) +
                   fetch_recover(nodes=False) + raceline.fan_order's classes and a NumPy lexsort pick
  one_q*_k*        Plan.recover + fetch_recover(nodes=False) with Q queries and one length: the floor

"kernel_ms" is rl_plan_kernel_ms(15) (the fan's two kernels) or (14) (the recover kernel) of the
same call: device time, upload and download excluded.  "host_ms" is the host clock around the
whole call, which ends after the fetch (it synchronises) and, for qc_*, after the pick.  The
expectation to confirm or refute: the fan's device time stays near one recover pass while the
candidates fit the device at once, and its call beats the Q*C route.

  python scripts/bench_recover_fan.py [--calls 20] [--out profiles/recover_fan_c2.json]
"""
import numpy as np

import stage_bench as sb
from stage_bench import abi

K_CAP = abi.RL_RCV_MAX_NODES
LENS = {c: np.geomspace(4.0, 120.0, c) for c in (4, 16)}


def tables(a):
    """(shapes, floors): name -> (q, c, k) of the fan_ and qc_ variants, name -> (q, k) of the one_ variants."""
    poses = ("q1", f"q{a.queries}")
    return ({f"{q}_c{c}_k{k}": (q, c, k) for q in poses for c in LENS for k in (64, K_CAP)},
            {f"{q}_k{k}": (q, k) for q in poses for k in (64, K_CAP)})


def variants(a):
    shapes, floors = tables(a)
    return [f"{kind}_{s}" for s in shapes for kind in ("fan", "qc")] + [f"one_{s}" for s in floors]


def host_pick(r, Q, C):
    """The winner of every pose from a recover answer of Q*C queries, in the fan stage's order."""
    fe, cl, mn, te = (x.reshape(Q, C) for x in (r.feasible, r.clamped, r.merge_node, r.t_end))
    cls = np.where(fe == 0, 3, np.where(mn < 0, 2, np.where(cl != 0, 1, 0)))     # raceline.fan_order's classes, vectorised
    idx = np.broadcast_to(np.arange(C), (Q, C))
    order = np.lexsort((idx, te, np.isnan(te), cls), axis=1)       # the last key is the first in the order
    return order[:, 0].astype(np.int32)


def main():
    a = sb.parse(sb.parser("bench_recover_fan", cap=64, queries=True), variants)
    c2 = sb.c2_setup(a, "mintime", bounds=True)
    pl, prob, cfg, rows, h, stamps, bnd = c2
    shapes, floors = tables(a)
    poses, dirs = (dict(zip(("q1", f"q{a.queries}"), x)) for x in sb.beside_poses(rows, bnd, prob, a.queries, K_CAP))
    own = {q: sb.own_speed(c2, P, a.dt)[0] for q, P in poses.items()}

    def call(v):
        kind, s = v.split("_", 1)
        if kind == "fan":
            q, c, k = shapes[s]
            pl.recover_fan(poses[q], own[q], cfg, LENS[c], dirs[q], dt=a.dt, m_cap=a.cap, k_cap=k)
            return pl.fetch_recover_fan(nodes=False)
        if kind == "qc":
            q, c, k = shapes[s]
            Q = poses[q].shape[0]
            pl.recover(np.repeat(poses[q], c, axis=0), np.repeat(own[q], c), cfg, np.tile(LENS[c], Q), np.repeat(dirs[q], c, axis=0),
                       dt=a.dt, m_cap=a.cap, k_cap=k)
            r = pl.fetch_recover(nodes=False)
            return r, host_pick(r, Q, c)
        q, k = floors[s]
        pl.recover(poses[q], own[q], cfg, 25.0, dirs[q], dt=a.dt, m_cap=a.cap, k_cap=k)
        return pl.fetch_recover(nodes=False)

    t, res = sb.interleave(pl, variants(a), call, lambda v: 15 if v.startswith("fan_") else 14, a.calls, a.warmup)
    pl.close()
    rec = {**sb.header(a, prob.N, "mintime"), "K_cap_max": K_CAP, "Q_many": a.queries, "calls_per_variant": a.calls,
           "warmup_calls": a.warmup, "h_m": float(h),
           "merge_lens_m": {f"c{c}": [round(float(x), 4) for x in v] for c, v in LENS.items()},
           "dir": "the raceline's heading + 10 degrees", "query_cfg": "the plan's", **sb.blocks(t)}
    for s, (q, c, k) in shapes.items():
        fan, (r, pick) = res[f"fan_{s}"], res[f"qc_{s}"]
        Q = poses[q].shape[0]
        win = np.arange(Q) * c + pick
        tick = np.arange(a.cap)[None, :] < fan.count[:, None]      # (ticks m >= count are unspecified)
        same = np.array_equal(fan.best, pick) and all(
            np.array_equal(getattr(fan, f).view(np.uint8), getattr(r, f)[win].view(np.uint8))
            for f in abi.HZN_LOC + abi.RCV_SCAL + abi.RCV_INTS) and all(
            np.array_equal(getattr(fan, f)[tick].view(np.uint8), getattr(r, f)[win][tick].view(np.uint8))
            for f in abi.TRAJ_COLS + abi.RCV_COLS)
        rec[f"equal_{s}"] = bool(same)                             # the fan's winner is the Q*C route's, bit for bit
        rec[f"best_hist_{s}"] = np.bincount(fan.best, minlength=c).tolist()
        rec[f"class_hist_{s}"] = np.bincount(fan.cand_class.ravel(), minlength=4).tolist()
        fk, qk, ok = rec[f"fan_{s}"], rec[f"qc_{s}"], rec[f"one_{q}_k{k}"]
        rec[f"fan_over_one_kernel_{s}"] = round(fk["kernel_ms"]["median"] / ok["kernel_ms"]["median"], 3)
        rec[f"fan_over_qc_kernel_{s}"] = round(fk["kernel_ms"]["median"] / qk["kernel_ms"]["median"], 3)
        rec[f"fan_over_qc_call_{s}"] = round(fk["host_ms"]["median"] / qk["host_ms"]["median"], 3)
    sb.write(a, "variants interleaved call by call in one process in a rotating order, warm-up calls dropped; host clock around "
                "Plan.recover_fan + fetch_recover_fan, around Plan.recover of Q*C queries + fetch_recover + the host pick, and "
                "around Plan.recover of Q queries + fetch_recover (the fetches synchronise; none downloads node arrays); "
                "rl_plan_kernel_ms(15) / (14) of the same call", [rec])
    sb.summarise(rec)


if __name__ == "__main__":
    main()
