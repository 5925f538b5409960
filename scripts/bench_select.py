"""Best-of-batch call against the full download, on the GPU, in one process.

Two workloads: C2 (competition_map1, N=2000, B=1024 seeds, min-curvature, 14 outer
iterations) and a C3-shaped min-time batch (N=2000, max_vpass_iters=20, B=512).  For each,
two variants are interleaved call by call (>= 20 calls each after warm-up):

  full   optimize_batch(out=reused)   every row of the batch downloaded (the existing path)
  best   optimize_best(k=1)           score, rank and gather on the device, one row downloaded

Both are synchronous host-in / host-out calls, so the host clock around a call is its
time; the in-call figures are the library's own (rl_last_call_times: HIP-event kernel time
and the call's wall time).  The selection stage's device time comes from a plan of the same
shape (rl_plan_kernel_ms index 3, HIP events around the three kernels).  The baseline is the
full-download call of this same process, never a number from another run.

  python scripts/bench_select.py [--calls 24] [--out profiles/select_c2.json]
"""
import json
import statistics
import time

import numpy as np

import stage_bench as sb
from stage_bench import abi, last_call, raceline


def stats(v):
    """stage_bench.stats' with the 10th and the 90th percentile."""
    v = sorted(v)
    return {"median": round(statistics.median(v), 4), "min": round(v[0], 4), "max": round(v[-1], 4),
            "p10": round(v[len(v) // 10], 4), "p90": round(v[(9 * len(v)) // 10], 4), "n": len(v)}


def workload(lib, label, case_name, B, mode, calls, warmup):
    prob, cfg = sb.problem(case_name)
    seeds = np.arange(B, dtype=np.uint64)
    mt = mode == "mintime"
    bit = abi.RL_MODE_MINTIME if mt else abi.RL_MODE_MINCURV
    lib.rl_release_plan_cache()
    out = raceline.optimize_batch(prob, cfg, seeds=seeds, B=B, mincurv=not mt, mintime=mt)
    t = {"full": {"host_ms": [], "call_ms": [], "kernel_ms": []}, "best": {"host_ms": [], "call_ms": [], "kernel_ms": []}}
    best = None
    for i in range(warmup + calls):
        for variant in ("full", "best"):
            t0 = time.perf_counter()
            if variant == "full":
                raceline.optimize_batch(prob, cfg, seeds=seeds, B=B, mincurv=not mt, mintime=mt, out=out)
            else:
                best = raceline.optimize_best(prob, cfg, seeds=seeds, B=B, mode=mode, k=1)
            host = (time.perf_counter() - t0) * 1e3
            k, c = last_call(lib)
            if i >= warmup:
                t[variant]["host_ms"].append(host)
                t[variant]["call_ms"].append(c)
                t[variant]["kernel_ms"].append(k)
    # the winner of the compact call is the winner of the full download (same plan, same kernel)
    full = out[1] if mt else out[0]
    b = int(best.index[0, 0])
    same = bool(np.array_equal(best.out.x[0], full.x[b]) and np.array_equal(best.out.kappa[0], full.kappa[b]))
    host_rank = int(np.lexsort((np.arange(B), best.scores, np.isnan(best.scores)))[0])
    # the selection stage alone, on a plan of the same shape
    pl = raceline.Plan(prob, cfg, seeds=seeds, B=B, modes=bit)
    sel_ms, opt_ms = [], []
    for _ in range(warmup + 5):
        pl.run()
        pl.select(bit, k=1)
        sel_ms.append(pl.kernel_ms(3))
        opt_ms.append(pl.kernel_ms(2 if mt else 1))
    pl.close()
    sel_ms, opt_ms = sel_ms[warmup:], opt_ms[warmup:]
    rec = {"workload": label, "case": case_name, "N": prob.N, "B": B, "mode": mode, "k": 1,
           "max_outer_iters": int(cfg.max_outer_iters), "calls_per_variant": calls, "warmup_calls": warmup,
           "full_download_bytes": int(sum(getattr(full, f).nbytes for f in abi.OUT_F64 + (("v", "ax", "lap", "vpass_sweeps") if mt else ())
                                          ) + full.evals.nbytes + full.accepts.nbytes),
           "best_download_bytes": int(best.index.nbytes + best.score.nbytes + best.scores.nbytes
                                      + sum(getattr(best.out, f).nbytes for f in abi.OUT_F64 + (("v", "ax", "lap", "vpass_sweeps") if mt else ()))
                                      + best.out.evals.nbytes + best.out.accepts.nbytes)}
    for variant in ("full", "best"):
        rec[variant] = {k: stats(v) for k, v in t[variant].items()}
    fm, bm = rec["full"]["call_ms"]["median"], rec["best"]["call_ms"]["median"]
    rec["best_call_over_full_call"] = round(bm / fm, 4)
    rec["best_call_minus_kernel_ms"] = round(bm - rec["best"]["kernel_ms"]["median"], 4)
    rec["full_call_minus_kernel_ms"] = round(fm - rec["full"]["kernel_ms"]["median"], 4)
    rec["selection_stage_ms"] = stats(sel_ms)
    rec["optimiser_kernel_ms_plan"] = stats(opt_ms)
    rec["selection_over_optimiser_kernel"] = round(statistics.median(sel_ms) / statistics.median(opt_ms), 6)
    rec["winner"] = {"index": b, "score": float(best.score[0, 0]), "host_argmin_of_device_scores": host_rank,
                     "rows_equal_full_download": same}
    return rec


def main():
    a = sb.parse(sb.parser("bench_select", calls=24, case=False), lambda a: ("full", "best"))
    lib = a.lib
    recs = [workload(lib, "C2", "cmap1_n2000", 1024, "mincurv", a.calls, a.warmup),
            workload(lib, "C3-shaped min-time", "cmap1_n2000_vp20", 512, "mintime", a.calls, a.warmup)]
    sb.write(a, "variants interleaved call by call in one process; host clock "
                "around synchronous calls, rl_last_call_ms for the in-call kernel (HIP events) and call time, "
                "rl_plan_kernel_ms(3) for the selection stage", recs)
    for r in recs:
        print(json.dumps({k: r[k] for k in ("workload", "best_call_over_full_call", "best_call_minus_kernel_ms",
                                            "full_call_minus_kernel_ms", "selection_over_optimiser_kernel", "winner")}
                         | {"full_call_ms": r["full"]["call_ms"]["median"], "best_call_ms": r["best"]["call_ms"]["median"],
                            "full_kernel_ms": r["full"]["kernel_ms"]["median"],
                            "best_kernel_ms": r["best"]["kernel_ms"]["median"]}))


if __name__ == "__main__":
    main()
