"""Several merge lengths per pose: the fan stage against the route it replaces (the recover stage
with Q*C queries and a pick on the host) and against one recover stage of Q queries, on the GPU,
in one process.

Set-up: bench_recover.py's: workload C2's plan (competition_map1, N=2000, B=1024 seeds, 14 outer
iterations), run once, the winner selected by lap, its trajectory stage (dt = 0.05 s, M_cap = 1024)
and its bounds stage resident; M_cap = 64 ticks, 0.05 s apart, every pose at the raceline's own
speed, the plan's cfg, the car heading 10 degrees left of the raceline; one pose 0.3 m beside the
line and 1024 poses jittered around it.  The C merge lengths are spaced geometrically from 4 m to
120 m.  The variants are interleaved call by call, in an order that rotates from round to round
(>= 20 calls each after warm-up, the warm-up calls dropped), and reported as medians with min-max:

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
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import oracle_lib as O  # noqa: E402  (fixture loader only)
from practice_path_planning_for_formula_student_driverless_amd import abi, raceline  # noqa: E402


def stats(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}


def host_pick(r, Q, C):
    """The winner of every pose from a recover answer of Q*C queries, in the fan stage's order."""
    fe, cl, mn, te = (x.reshape(Q, C) for x in (r.feasible, r.clamped, r.merge_node, r.t_end))
    cls = np.where(fe == 0, 3, np.where(mn < 0, 2, np.where(cl != 0, 1, 0)))     # raceline.fan_order's classes, vectorised
    idx = np.broadcast_to(np.arange(C), (Q, C))
    order = np.lexsort((idx, te, np.isnan(te), cls), axis=1)       # the last key is the first in the order
    return order[:, 0].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", default="cmap1_n2000")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "recover_fan_c2.json"))
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls: at least 20 per variant")
    lib = abi.load_library()
    if lib.rl_device_count() < 1:
        raise SystemExit("bench_recover_fan: no HIP device visible (nothing is measured without one)")
    case = O.load_case(a.case)
    prob, cfg = O.case_problem(case), O.case_cfg(case)
    B, N = a.batch, prob.N
    K_CAP = abi.RL_RCV_MAX_NODES
    pl = raceline.Plan(prob, cfg, seeds=np.arange(B, dtype=np.uint64), B=B, modes=abi.RL_MODE_MINTIME)
    pl.run()
    pl.select("mintime", k=1, score="lap")
    pl.trajectory("mintime", a.dt, 1024, rows="selected")
    pl.bounds()
    sel, traj, bnd = pl.fetch_selected(), pl.fetch_trajectory(), pl.fetch_bounds()
    o = sel.out
    rows, h = (o.x, o.y, o.heading, o.kappa, o.v, o.ax), prob.L / N
    rng = np.random.default_rng(1)
    at1 = np.array([N // 3])
    at = rng.integers(0, N - 1 - K_CAP if not prob.closed else N, size=a.queries)

    def beside(at, e):
        return np.ascontiguousarray(np.stack([rows[0][0, at] + e * bnd.nx[0, at], rows[1][0, at] + e * bnd.ny[0, at]], axis=1))

    def heading(at):
        psi = rows[2][0, at] + np.pi / 18.0
        return np.ascontiguousarray(np.stack([np.cos(psi), np.sin(psi)], axis=1))

    poses = {"q1": beside(at1, 0.3), f"q{a.queries}": beside(at, rng.uniform(-0.6, 0.6, size=a.queries))}
    dirs = {"q1": heading(at1), f"q{a.queries}": heading(at)}
    own = {}
    for q, P in poses.items():          # the raceline's own speed at the located points
        hz = raceline.horizon_host(*rows, h, prob.closed, P, dt=a.dt, m_cap=1, stamps=traj.stamps)
        V = rows[4][0]
        own[q] = V[hz.seg] + hz.u * (V[(hz.seg + 1) % N] - V[hz.seg])
    lens = {c: np.geomspace(4.0, 120.0, c) for c in (4, 16)}

    shapes = {f"{q}_c{c}_k{k}": (q, c, k) for q in poses for c in lens for k in (64, K_CAP)}
    floors = {f"{q}_k{k}": (q, k) for q in poses for k in (64, K_CAP)}
    names = [f"{kind}_{s}" for s in shapes for kind in ("fan", "qc")] + [f"one_{s}" for s in floors]
    t = {v: {"host_ms": [], "kernel_ms": []} for v in names}
    res = {}
    for i in range(a.warmup + a.calls):
        for v in names[i % len(names):] + names[:i % len(names)]:   # (what a variant follows changes from call to call)
            kind, s = v.split("_", 1)
            t0 = time.perf_counter()
            if kind == "fan":
                q, c, k = shapes[s]
                pl.recover_fan(poses[q], own[q], cfg, lens[c], dirs[q], dt=a.dt, m_cap=a.cap, k_cap=k)
                res[v] = pl.fetch_recover_fan(nodes=False)
            elif kind == "qc":
                q, c, k = shapes[s]
                Q = poses[q].shape[0]
                pl.recover(np.repeat(poses[q], c, axis=0), np.repeat(own[q], c), cfg, np.tile(lens[c], Q), np.repeat(dirs[q], c, axis=0),
                           dt=a.dt, m_cap=a.cap, k_cap=k)
                r = pl.fetch_recover(nodes=False)
                res[v] = (r, host_pick(r, Q, c))
            else:
                q, k = floors[s]
                pl.recover(poses[q], own[q], cfg, 25.0, dirs[q], dt=a.dt, m_cap=a.cap, k_cap=k)
                res[v] = pl.fetch_recover(nodes=False)
            ms = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                t[v]["host_ms"].append(ms)
                t[v]["kernel_ms"].append(pl.kernel_ms(15 if kind == "fan" else 14))
    pl.close()
    rec = {"workload": "C2", "case": a.case, "N": N, "B": B, "mode": "mintime", "dt": a.dt, "M_cap": a.cap, "K_cap_max": K_CAP,
           "Q_many": a.queries, "calls_per_variant": a.calls, "warmup_calls": a.warmup, "h_m": float(h),
           "merge_lens_m": {f"c{c}": [round(float(x), 4) for x in v] for c, v in lens.items()},
           "dir": "the raceline's heading + 10 degrees", "query_cfg": "the plan's"}
    for v in names:
        rec[v] = {k: stats(x) for k, x in t[v].items()}
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
    doc = {"script": "scripts/bench_recover_fan.py",
           "method": "variants interleaved call by call in one process in a rotating order, warm-up calls dropped; host clock around "
                     "Plan.recover_fan + fetch_recover_fan, around Plan.recover of Q*C queries + fetch_recover + the host pick, and "
                     "around Plan.recover of Q queries + fetch_recover (the fetches synchronise; none downloads node arrays); "
                     "rl_plan_kernel_ms(15) / (14) of the same call",
           "records": [rec]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k not in ("workload", "case")}))


if __name__ == "__main__":
    main()
