"""The free track width along the raceline: the bounds stage and its tick kernel against the route
through the host, on the GPU, in one process.

Set-up: workload C2's plan (competition_map1, N=2000, B=1024 seeds, 14 outer iterations), run
once.  Phase 1: the winner selected by lap and its trajectory stage resident (R = 1).  Phase 2: the
trajectory stage of all 1 024 rows.  Within a phase the variants are interleaved call by call, in
stage_bench.rounds' rotating order (>= 20 calls each after warm-up, the warm-up calls dropped),
and reported as medians with min-max:

  bnd_r1, bnd_r1024     Plan.bounds + fetch_bounds (lo, hi, nx, ny) of the winner / of all rows
  hb_q1, hb_q1024       Plan.horizon_bounds + fetch_horizon_bounds at the ticks of a resident
                        horizon stage of 1 / 1024 poses on the winner (M_cap = 64, dt = 0.05 s)
  host_r1, host_r1024   the route through the host: download the rows (fetch_selected / fetch),
                        then raceline.corridor about each row, which uploads the rings per call
                        (host_r1024: --host-calls calls, it takes seconds)

The host clock around a device variant ends after the fetch, which synchronises;
rl_plan_kernel_ms(11) / (12) is the stage's device time of the same call.  No target is set.

  python scripts/bench_bounds.py [--mode mintime] [--calls 20] [--out profiles/bounds_c2.json]
"""
import time

import numpy as np

import stage_bench as sb
from stage_bench import abi, raceline


def phase1(a):
    return ["bnd_r1", "hb_q1", f"hb_q{a.queries}", "host_r1"]


def variants(a):
    return phase1(a) + [f"bnd_r{a.batch}"] + ([f"host_r{a.batch}"] if a.host_calls else [])


def bits_equal(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)))


def host_route(prob, cfg, o):
    """raceline.corridor about every row of o: (lo, hi) [R, N]."""
    out = [raceline.corridor(abi.Problem(center=np.stack([o.x[r], o.y[r]], axis=1), L=prob.L, inner_seg=prob.inner_seg,
                                         outer_seg=prob.outer_seg, veh_width=prob.veh_width, closed=prob.closed), cfg)
           for r in range(o.x.shape[0])]
    return np.stack([c[0] for c in out]), np.stack([c[1] for c in out])


def main():
    ap = sb.parser("bench_bounds", mode="mintime", cap=64, queries=True)
    ap.add_argument("--host-calls", type=int, default=3)
    a = sb.parse(ap, variants)
    # ---- phase 1: the winner
    c2 = sb.c2_setup(a, a.mode, bounds=True)
    pl, prob, cfg, rows = c2[:4]
    B, mt = a.batch, a.mode == "mintime"
    t, res = {}, {}

    def clock(v, i, fn, idx=None):
        t.setdefault(v, {"host_ms": []})
        t0 = time.perf_counter()
        res[v] = fn()
        ms = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            t[v]["host_ms"].append(ms)
            if idx is not None:
                t[v].setdefault("kernel_ms", []).append(pl.kernel_ms(idx))

    def stage():
        pl.bounds()
        return pl.fetch_bounds()

    def ticks():
        pl.horizon_bounds()
        return pl.fetch_horizon_bounds()

    poses = dict(zip(("q1", f"q{a.queries}"), sb.jittered_poses(rows[0], rows[1], prob, a.queries)))
    for i, v in sb.rounds(phase1(a), a.warmup + a.calls):
        if v == "bnd_r1":
            clock(v, i, stage, 11)
        elif v == "host_r1":
            clock(v, i, lambda: host_route(prob, cfg, pl.fetch_selected().out))
        else:
            pl.horizon(poses[v[3:]], dt=a.dt, m_cap=a.cap)      # (the bounds stage above made the ticks' bounds stale)
            pl.fetch_horizon()
            clock(v, i, ticks, 12)
    rec = {**sb.header(a, prob.N, a.mode), "Q_many": a.queries, "calls_per_variant": a.calls, "warmup_calls": a.warmup,
           "veh_width": prob.veh_width, "margin": cfg.safety_margin_m}
    rec["bit_equal_r1"] = bits_equal(res["bnd_r1"].lo, res["host_r1"][0]) and bits_equal(res["bnd_r1"].hi, res["host_r1"][1])
    # ---- phase 2: all rows
    pl.trajectory(a.mode, a.dt, 16, rows="all")
    for i in range(a.warmup + a.calls):
        clock(f"bnd_r{B}", i, stage, 11)
    for i in range(a.host_calls):
        clock(f"host_r{B}", a.warmup + i, lambda: host_route(prob, cfg, pl.fetch()[1 if mt else 0]))
    rec[f"bit_equal_r{B}"] = (bits_equal(res[f"bnd_r{B}"].lo, res[f"host_r{B}"][0]) and
                              bits_equal(res[f"bnd_r{B}"].hi, res[f"host_r{B}"][1])) if a.host_calls else None
    pl.close()
    rec.update(sb.blocks(t))
    for r in (1, B):
        if f"host_r{r}" in rec:
            rec[f"dev_over_host_r{r}"] = round(rec[f"bnd_r{r}"]["host_ms"]["median"] / rec[f"host_r{r}"]["host_ms"]["median"], 6)
    rec["us_per_row_r%d" % B] = round(rec[f"bnd_r{B}"]["kernel_ms"]["median"] * 1e3 / B, 4)
    sb.write(a, "variants interleaved call by call in one process in a rotating order, warm-up calls dropped; host clock around "
                "Plan.bounds + fetch_bounds / Plan.horizon_bounds + fetch_horizon_bounds (which synchronise) and around the "
                "download of the rows plus raceline.corridor per row; rl_plan_kernel_ms(11) / (12) of the same call", [rec])
    sb.summarise(rec)


if __name__ == "__main__":
    main()
