"""Ranking a min-curvature batch by lap time: the lap stage against the host route, on the
GPU, in one process.

Workload C2 (competition_map1, N=2000, B=1024 seeds, min-curvature, 14 outer iterations).
Three variants are interleaved call by call (>= 20 calls each after warm-up):

  route    optimize_batch(out=reused) -> path_length per row on the host -> lap_eval of all
           rows -> rank_scores: the way to the fastest min-curvature raceline without the stage
  lap      optimize_best(mode="mincurv", k=1, score="lap"): the lap stage and the selection on
           the device, one row downloaded
  default  optimize_best(mode="mincurv", k=1): the same call ranked by h * sum kappa^2

All are synchronous host-in / host-out calls, so the host clock around a variant is its time;
the in-call figures are the library's own (rl_last_call_ms after the optimiser call: HIP-event
time of the run and the call's wall time).  The lap stage's device time comes from a plan of
the same shape (rl_plan_kernel_ms 4 = the stage, 5 = its preparation kernel, 6 = its
evaluation kernel, 3 = the selection, 1 = the optimiser).  Bytes moved are counted from the
arrays each variant passes.  A second loop interleaves the two best-of calls with each other
only ("pair_only"): in the first loop they run behind the route's second of host work, on a
GPU that has been idle.

  python scripts/bench_lap_select.py [--calls 20] [--out profiles/lap_select_c2.json]
"""
import ctypes as C
import json
import time

import numpy as np

import stage_bench as sb
from stage_bench import abi, last_call, raceline, stats


def variants(a):
    return ["route", "lap", "default"]


def main():
    a = sb.parse(sb.parser("bench_lap_select"), variants)
    lib = a.lib
    prob, cfg = sb.problem(a.case)
    B, N = a.batch, prob.N
    seeds = np.arange(B, dtype=np.uint64)
    MC = abi.RL_MODE_MINCURV
    lib.rl_release_plan_cache()
    out = raceline.optimize_batch(prob, cfg, seeds=seeds, B=B, mincurv=True, mintime=False)
    names = variants(a)
    t = {v: {"host_ms": [], "call_ms": [], "kernel_ms": []} for v in names}
    parts = {"optimize_batch_ms": [], "path_length_ms": [], "lap_eval_ms": [], "rank_scores_ms": []}
    res = {}
    for i in range(a.warmup + a.calls):
        for variant in names:
            t0 = time.perf_counter()
            if variant == "route":
                raceline.optimize_batch(prob, cfg, seeds=seeds, B=B, mincurv=True, mintime=False, out=out)
                k, c = last_call(lib)
                t1 = time.perf_counter()
                mc = out[0]
                Ls = np.array([raceline.path_length(np.column_stack([mc.x[b], mc.y[b]]), prob.closed) for b in range(B)])
                t2 = time.perf_counter()
                ev = raceline.lap_eval(np.stack([mc.x, mc.y], axis=2), Ls, prob.closed, cfg)
                t3 = time.perf_counter()
                idx = raceline.rank_scores(ev.lap, 1)
                t4 = time.perf_counter()
                res["route"] = (int(idx[0, 0]), ev.lap.copy(), Ls)
                if i >= a.warmup:
                    for name, d in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                        parts[name].append(d * 1e3)
            else:
                sel = raceline.optimize_best(prob, cfg, seeds=seeds, B=B, mode="mincurv", k=1,
                                             score="lap" if variant == "lap" else "default")
                k, c = last_call(lib)
                res[variant] = sel
            host = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                t[variant]["host_ms"].append(host)
                t[variant]["call_ms"].append(c)
                t[variant]["kernel_ms"].append(k)
    # the two best-of calls alone, interleaved with each other only: in the loop above each of
    # them follows a variant that leaves the GPU idle for the host's path lengths (about a
    # second) or follows the call that did, so its kernel starts on a GPU that has clocked down
    pair = ("lap", "default")
    t2 = {v: {"host_ms": [], "call_ms": [], "kernel_ms": []} for v in pair}
    for i in range(a.warmup + a.calls):
        for variant in pair:
            t0 = time.perf_counter()
            raceline.optimize_best(prob, cfg, seeds=seeds, B=B, mode="mincurv", k=1,
                                   score="lap" if variant == "lap" else "default")
            host = (time.perf_counter() - t0) * 1e3
            k, c = last_call(lib)
            if i >= a.warmup:
                t2[variant]["host_ms"].append(host)
                t2[variant]["call_ms"].append(c)
                t2[variant]["kernel_ms"].append(k)
    # the stage alone, on a plan of the same shape
    pl = raceline.Plan(prob, cfg, seeds=seeds, B=B, modes=MC)
    st = {"lap_stage_ms": [], "prep_ms": [], "evaluation_ms": [], "selection_ms": [], "optimiser_kernel_ms": []}
    for j in range(a.warmup + 10):
        pl.run()
        pl.select(MC, k=1, score="lap")
        ms = [pl.kernel_ms(q) for q in (4, 5, 6, 3, 1)]
        if j >= a.warmup:
            for name, v in zip(st, ms):
                st[name].append(v)
    pl.close()
    mc = out[0]
    bn8 = B * N * 8
    lap_sel = res["lap"]
    best_rows = (lap_sel.index.nbytes + lap_sel.score.nbytes + lap_sel.scores.nbytes
                 + sum(getattr(lap_sel.out, f).nbytes for f in abi.OUT_F64 + ("v", "ax", "lap", "vpass_sweeps"))
                 + lap_sel.out.evals.nbytes + lap_sel.out.accepts.nbytes)
    dflt = res["default"]
    default_rows = (dflt.index.nbytes + dflt.score.nbytes + dflt.scores.nbytes
                    + sum(getattr(dflt.out, f).nbytes for f in abi.OUT_F64) + dflt.out.evals.nbytes + dflt.out.accepts.nbytes)
    up_common = prob.center.nbytes + C.sizeof(abi.RlCfg) + seeds.nbytes
    ridx, rlap, rL = res["route"]
    rec = {"workload": "C2", "case": a.case, "N": N, "B": B, "mode": "mincurv", "k": 1,
           "max_outer_iters": int(cfg.max_outer_iters), "calls_per_variant": a.calls, "warmup_calls": a.warmup,
           "bytes": {"route": {"download": 6 * bn8 + mc.evals.nbytes + mc.accepts.nbytes + 4 * bn8 + B * 8 + B * 4 + 4,
                               "upload": up_common + 2 * bn8 + B * 8 + C.sizeof(abi.RlCfg) + B * 8},
                     "lap": {"download": best_rows, "upload": up_common},
                     "default": {"download": default_rows, "upload": up_common}}}
    rec.update(sb.blocks(t))
    rec["route_parts_host_ms"] = {k: stats(v) for k, v in parts.items()}
    rec["pair_only"] = sb.blocks(t2)
    rec["pair_only"]["lap_minus_default_call_ms"] = round(rec["pair_only"]["lap"]["call_ms"]["median"]
                                                          - rec["pair_only"]["default"]["call_ms"]["median"], 4)
    rec["pair_only"]["lap_minus_default_kernel_ms"] = round(rec["pair_only"]["lap"]["kernel_ms"]["median"]
                                                            - rec["pair_only"]["default"]["kernel_ms"]["median"], 4)
    rec["plan"] = {k: stats(v) for k, v in st.items()}
    med = sb.medians(rec)
    rec["lap_minus_default_call_ms"] = round(med("lap", "call_ms") - med("default", "call_ms"), 4)
    rec["lap_minus_default_host_ms"] = round(med("lap", "host_ms") - med("default", "host_ms"), 4)
    rec["lap_over_route_host"] = round(med("lap", "host_ms") / med("route", "host_ms"), 6)
    rec["stage_over_optimiser_kernel"] = round(rec["plan"]["lap_stage_ms"]["median"]
                                               / rec["plan"]["optimiser_kernel_ms"]["median"], 6)
    b = int(lap_sel.index[0, 0])
    rec["winner"] = {"index_lap": b, "lap_s": float(lap_sel.score[0, 0]), "index_route": ridx,
                     "lap_bits_equal_route": bool(np.array_equal(lap_sel.scores.view(np.uint64), rlap.view(np.uint64))),
                     "rows_equal_full_download": bool(np.array_equal(lap_sel.out.x[0], mc.x[b])
                                                      and np.array_equal(lap_sel.out.kappa[0], mc.kappa[b])),
                     "index_default_score": int(dflt.index[0, 0]),
                     "lap_of_default_winner_s": float(lap_sel.scores[int(dflt.index[0, 0])])}
    sb.write(a, "variants interleaved call by call in one process; host clock around each variant, "
                "rl_last_call_ms after the optimiser call for the in-call kernel (HIP events: the run, without "
                "the stages after it) and call time; rl_plan_kernel_ms(4, 5, 6, 3, 1) on a plan of the same shape "
                "for the lap stage, its two kernels, the selection and the optimiser; pair_only: lap and default "
                "interleaved without the route between them", [rec])
    print(json.dumps({k: rec[k] for k in ("lap_minus_default_call_ms", "lap_minus_default_host_ms", "lap_over_route_host",
                                          "stage_over_optimiser_kernel", "winner", "plan", "route_parts_host_ms", "pair_only")}
                     | {v + "_host_ms": rec[v]["host_ms"] for v in names}
                     | {v + "_call_ms": rec[v]["call_ms"] for v in names}
                     | {v + "_kernel_ms": rec[v]["kernel_ms"] for v in names}))


if __name__ == "__main__":
    main()
