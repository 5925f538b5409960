"""The winner of a batch as a time-stamped trajectory: the trajectory stage against resampling
on the host, on the GPU, in one process.

Workload C2 (competition_map1, N=2000, B=1024 seeds, 14 outer iterations), ticks of
dt = 0.05 s, at most M_cap = 1024 per row.  Three variants are interleaved call by call
(>= 20 calls each after warm-up, the warm-up calls dropped):

  host   optimize_batch(out=reused), every row downloaded, then raceline.trajectory_host of the
         winner.  mintime: the winner is the argmin of the downloaded laps.  mincurv: the rows
         carry no speed, so the winner's index is taken from the `best` variant for free, and
         its path length, lap_eval and trajectory_host follow on the host
  traj   best_trajectory(k=1, score="lap"): lap stage, selection and trajectory stage on the
         device; the winner's rows and ticks downloaded
  best   optimize_best(k=1, score="lap") alone: the same call without the trajectory

All are synchronous host-in / host-out calls, so the host clock around a variant is its time;
rl_last_call_ms gives the library's own wall time of the optimiser call.  The stage's device
time comes from a plan of the same shape: rl_plan_kernel_ms 7 after rows="all" and after
rows="selected", against the optimiser kernel (index 1 or 2).  The stamp chain is serial in N;
its cost at N = 10^4 and beyond is not measured here.

  python scripts/bench_trajectory.py [--mode mincurv] [--calls 20] [--out profiles/trajectory_c2.json]
"""
import time

import numpy as np

import stage_bench as sb
from stage_bench import abi, last_call, raceline, stats


def variants(a):
    return ["host", "traj", "best"]


def host_winner(prob, cfg, out, mode, winner, dt, m_cap):
    """trajectory_host of the winner of a full download (mincurv: of row `winner`)."""
    if mode == "mintime":
        o = out[1]
        b = int(np.argmin(o.lap))
        return b, raceline.trajectory_host(o.x[b], o.y[b], o.heading[b], o.kappa[b], o.v[b], o.ax[b], prob.L / prob.N,
                                           prob.closed, dt, m_cap)
    o, b = out[0], winner
    path = np.column_stack([o.x[b], o.y[b]])
    Lb = raceline.path_length(path, prob.closed)
    ev = raceline.lap_eval(path, [Lb], prob.closed, cfg)
    return b, raceline.trajectory_host(o.x[b], o.y[b], ev.heading[0], ev.kappa[0], ev.v[0], ev.ax[0], Lb / prob.N,
                                       prob.closed, dt, m_cap)


def main():
    a = sb.parse(sb.parser("bench_trajectory", mode="mincurv", cap=1024), variants)
    lib = a.lib
    prob, cfg = sb.problem(a.case)
    B, N, mode, dt, cap = a.batch, prob.N, a.mode, a.dt, a.cap
    mt = mode == "mintime"
    seeds = np.arange(B, dtype=np.uint64)
    lib.rl_release_plan_cache()
    out = raceline.optimize_batch(prob, cfg, seeds=seeds, B=B, mincurv=not mt, mintime=mt)
    winner = int(raceline.optimize_best(prob, cfg, seeds=seeds, B=B, mode=mode, k=1, score="lap").index[0, 0])
    names = variants(a)
    t = {v: {"host_ms": [], "call_ms": []} for v in names}
    parts = {"optimize_batch_ms": [], "resample_on_host_ms": []}
    res = {}
    for i in range(a.warmup + a.calls):
        for variant in names:
            t0 = time.perf_counter()
            if variant == "host":
                raceline.optimize_batch(prob, cfg, seeds=seeds, B=B, mincurv=not mt, mintime=mt, out=out)
                _, c = last_call(lib)
                t1 = time.perf_counter()
                res["host"] = host_winner(prob, cfg, out, mode, winner, dt, cap)
                if i >= a.warmup:
                    parts["optimize_batch_ms"].append((t1 - t0) * 1e3)
                    parts["resample_on_host_ms"].append((time.perf_counter() - t1) * 1e3)
            elif variant == "traj":
                res["traj"] = raceline.best_trajectory(prob, cfg, seeds=seeds, B=B, mode=mode, k=1, score="lap", dt=dt, m_cap=cap)
                _, c = last_call(lib)
            else:
                res["best"] = raceline.optimize_best(prob, cfg, seeds=seeds, B=B, mode=mode, k=1, score="lap")
                _, c = last_call(lib)
            if i >= a.warmup:
                t[variant]["host_ms"].append((time.perf_counter() - t0) * 1e3)
                t[variant]["call_ms"].append(c)
    # the stage alone, on a plan of the same shape
    pl = raceline.Plan(prob, cfg, seeds=seeds, B=B, modes=abi.RL_MODE_MINTIME if mt else abi.RL_MODE_MINCURV)
    st = {"optimiser_kernel_ms": [], "stage_all_ms": [], "stage_selected_ms": []}
    for j in range(a.warmup + 10):
        pl.run()
        pl.select(mode, k=1, score="lap")
        pl.trajectory(mode, dt, cap, rows="all")
        ms_all = pl.kernel_ms(7)
        pl.trajectory(mode, dt, cap, rows="selected")
        ms = (pl.kernel_ms(2 if mt else 1), ms_all, pl.kernel_ms(7))
        if j >= a.warmup:
            for name, v in zip(st, ms):
                st[name].append(v)
    pl.close()
    sel, traj = res["traj"]
    hb, htraj = res["host"]
    m = int(traj.count[0])
    equal = hb == int(sel.index[0, 0]) and m == int(htraj.count[0]) and all(
        np.array_equal(getattr(traj, f)[0, :m].view(np.uint64), getattr(htraj, f)[0, :m].view(np.uint64))
        for f in abi.TRAJ_COLS)
    rec = {"workload": "C2", "case": a.case, "N": N, "B": B, "mode": mode, "k": 1, "score": "lap", "dt": dt, "M_cap": cap,
           "max_outer_iters": int(cfg.max_outer_iters), "calls_per_variant": a.calls, "warmup_calls": a.warmup}
    rec.update(sb.blocks(t))
    rec["host_parts_ms"] = {k: stats(v) for k, v in parts.items()}
    rec["plan"] = {k: stats(v) for k, v in st.items()}
    med = sb.medians(rec)
    rec["traj_minus_best_call_ms"] = round(med("traj", "call_ms") - med("best", "call_ms"), 4)
    rec["traj_minus_best_host_ms"] = round(med("traj", "host_ms") - med("best", "host_ms"), 4)
    rec["best_call_ms_spread"] = round(rec["best"]["call_ms"]["max"] - rec["best"]["call_ms"]["min"], 4)
    rec["best_host_ms_spread"] = round(rec["best"]["host_ms"]["max"] - rec["best"]["host_ms"]["min"], 4)
    rec["traj_over_host_route"] = round(med("traj", "host_ms") / med("host", "host_ms"), 6)
    opt = rec["plan"]["optimiser_kernel_ms"]["median"]
    rec["stage_all_over_optimiser_kernel"] = round(rec["plan"]["stage_all_ms"]["median"] / opt, 6)
    rec["stage_selected_over_optimiser_kernel"] = round(rec["plan"]["stage_selected_ms"]["median"] / opt, 6)
    rec["winner"] = {"index": int(sel.index[0, 0]), "ticks": m, "T_s": float(traj.T[0]), "score_lap_s": float(sel.score[0, 0]),
                     "ticks_bit_equal_host": bool(equal)}
    sb.write(a, "variants interleaved call by call in one process, warm-up calls dropped; host clock around each "
                "variant, rl_last_call_ms after the optimiser call for its wall time inside the library; "
                "rl_plan_kernel_ms(7) after rows=all and rows=selected and the optimiser kernel on a plan of the same "
                "shape; the stamp chain at N >= 10^4 is not measured", [rec])
    sb.summarise(rec)


if __name__ == "__main__":
    main()
