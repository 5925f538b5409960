#!/usr/bin/env python3
"""The A/B harness of the experiment scripts: one workload table, one timing function, one
stamps / counters function (experiments only; bench.py is the product's measurement).

  ab.py --list                      the workloads and the variants of build_variants.VARIANTS
  ab.py time c5 [--variants 'bt*'] [--B 1024] [--modes 1] [--rounds 4]
  ab.py time c4 [--schedule each|streams|group] [--per-plan]      (AB_MODE=mc|mt, AB_PER_PLAN=1)
  ab.py time c2,c5 --inner 0        max_inner_iters = 0: the corridor phase alone (INNER=0)
  ab.py time all                    every workload (AB_CASES=c2,c3mt selects)
  ab.py time c2 --variants product --env RL_CORRIDOR0=1,0         one library under two environments
  ab.py run c5 [--inner default,0] [--launches 2]                 a few launches, for a profiler
  ab.py stamps c5 --mode 2 [--variant stamps_eval] [--seed0 0]    RL_STAMPS build (ST_CASES=...)
  ab.py counts c5 [--outer 1,2,14] [--corridor]                   RL_COUNT build (COUNT_CASE=...)

`time` loads the libraries of _lib/variants/ that match --variants (`product`: the product
library), creates every plan, runs --rounds rounds with the libraries interleaved inside each
round, drops the first round and prints median and minimum of rl_plan_kernel_ms per mode, of
the run bracket and, for concurrent schedules, of the wall time.  Then every library's outputs
are compared with the first one's over FIELDS: every rl_out member the mode produces.
"""
from __future__ import annotations

import argparse
import ctypes as C
import functools
import glob
import json
import os
import sys
import time
from contextlib import contextmanager
from dataclasses import dataclass, replace

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "scripts"), os.path.join(REPO, "tests"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import oracle_lib as O  # noqa: E402  (fixture loader only)
from build_variants import VARIANTS  # noqa: E402
from practice_path_planning_for_formula_student_driverless_amd import abi, raceline  # noqa: E402
from practice_path_planning_for_formula_student_driverless_amd import distributed as D  # noqa: E402

VARIANT_DIR = os.path.join(abi.PKG_DIR, "_lib", "variants")
DIAGNOSTIC = ("stamps", "stamps_eval", "count")      # variants that are read out, never timed
MC, MT = abi.RL_MODE_MINCURV, abi.RL_MODE_MINTIME
MODE_NAME = {MC: "min-curv", MT: "min-time"}
# the members of rl_out each mode produces, counters included: what "bit-exact" means here
FIELDS = {MC: abi.OUT_F64 + ("evals", "accepts"),
          MT: abi.OUT_F64_MT + ("lap", "evals", "accepts", "vpass_sweeps")}
TRACKS = tuple("track_" + t for t in D.C4_TRACKS)


@dataclass(frozen=True)
class Workload:
    cases: tuple                # fixtures of tests/golden (manifest.json "cases"), one problem each
    B: tuple = (1024,)          # batch sizes, one measurement each
    modes: tuple = (MC,)        # mode word of each plan of a case: (3,) one plan of both, (1, 2) two plans
    cfg: tuple = ()             # (field, value) overrides of the case's cfg
    seeds: bool = True          # seeds 0..B-1; False: none (the centre line)
    grid: bool = False          # cfgs = distributed.c4_cfgs (B sweep points); shape batch = all plans' instances
    open: bool = False          # the track as an open path (bench.open_problem)
    envs: tuple = ((),)         # environments ((name, value), ...) the plans are created and run under
    schedule: str = "each"      # each: one plan after the other; streams: all at once; group: rl_plan_run_group
    what: str = ""


_LAT = ((("RL_LAT_SHAPES", "1"),), (("RL_LAT_SHAPES", "0"),))
_STREAM = ((("RL_FORCE_STREAM", "1"),),)
WORKLOADS = {
    "c2": Workload(("cmap1_n2000",), what="competition_map1 N=2000, 1024 seeds, min-curvature"),
    "c3": Workload(("cmap1_n2000_vp20",), (256, 4096), (MC | MT,), what="C2's track, max_vpass_iters=20, one plan of both modes"),
    "c3mt": Workload(("cmap1_n2000_vp20",), (256, 4096), (MT,), what="C3's min-time alone"),
    "c4": Workload(TRACKS, (512,), (MC, MT), seeds=False, grid=True, schedule="streams",
                   what="7 bundled tracks x 512 (mu, P_max_W, lambda_smooth) points, one plan per (track, mode), as bench.run_c4"),
    "c4t": Workload(TRACKS, (512,), (MC | MT,), what="C4-shaped plans: each bundled track with its own cfg, 512 seeds, both modes"),
    "c4t3": Workload(("track_competition_map_testday3",), (512,), (MC | MT,), what="one C4-shaped plan (N=261)"),
    "c5": Workload(("oval_n10000",), what="oval N=10000, 1024 seeds, min-curvature (streaming kernel)"),
    "c5mt": Workload(("oval_n10000",), modes=(MT,), what="C5's problem, min-time"),
    "s2": Workload(("cmap1_n2000",), envs=_STREAM, what="C2's problem forced through the streaming kernel"),
    "s2mt": Workload(("cmap1_n2000",), modes=(MT,), envs=_STREAM, what="the same, min-time"),
    "o2": Workload(("cmap1_n2000",), open=True, what="C2's track as an open path"),
    "o2mt": Workload(("cmap1_n2000",), modes=(MT,), open=True, what="the same, min-time"),
    "lat": Workload(("track_training_map", "track_competition_map1", "track_competition_map_testday3", "cmap1_n2000"),
                    (1,), (MC, MT), seeds=False, envs=_LAT,
                    what="one track per call (drop-in): the latency shapes and, RL_LAT_SHAPES=0, the throughput shapes"),
}


# ------------------------------------------------------------------ libraries
def variant_path(name: str) -> str:
    return os.path.join(VARIANT_DIR, f"librl_{name}.so")


def find_libs(patterns: str = "*") -> dict:
    """name -> path of the libraries to compare, in order: `product` is the product library,
    every other comma-separated pattern globs _lib/variants/librl_<pattern>.so (the diagnostic
    builds are left out unless named exactly)."""
    libs = {}
    for pat in patterns.split(","):
        if pat == "product":
            libs["product"] = abi.LIB_PATH
            continue
        for p in sorted(glob.glob(variant_path(pat))):
            n = os.path.basename(p)[6:-3]
            if n not in DIAGNOSTIC or n == pat:
                libs[n] = p
    if not libs:
        sys.exit(f"ab.py: no library matches {patterns!r} in {VARIANT_DIR} (python scripts/build_variants.py NAME ...)")
    return libs


def load_library(path: str = abi.LIB_PATH):
    """abi.load_library after torch: the streams of the concurrent schedules are torch's, and
    torch finds no device once another copy of the HIP runtime has initialised in the process
    (bench.py imports torch first too)."""
    import torch  # noqa: F401

    return abi.load_library(path)


@contextmanager
def environ(env):
    """os.environ with the (name, value) pairs of env set; restored on exit."""
    env = dict(env)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------ plans
class LibPlan:
    """rl_plan_* of one library (raceline.Plan is bound to the product library)."""

    def __init__(self, lib, prob, cfgs, seeds, B: int, modes: int, label: str = ""):
        self.lib, self.B, self.N, self.modes, self.label = lib, B, prob.N, modes, label
        cfg_arr, ncfg = abi.cfg_array(cfgs)
        self.max_outer = int(cfg_arr[0].max_outer_iters)
        self._keep = (prob, cfg_arr)
        self.h = C.c_void_p()
        p = prob.as_c()
        self._check(lib.rl_plan_create(C.byref(self.h), 0, C.byref(p), cfg_arr, ncfg,
                                       abi.u64ptr(abi.seed_array(seeds)), B, modes), "rl_plan_create")

    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            raise RuntimeError(f"{what} = {rc}: {self.lib.rl_last_error().decode(errors='replace')}")

    def set_shape_batch(self, shape_B: int) -> None:
        self._check(self.lib.rl_plan_set_shape_batch(self.h, int(shape_B)), "rl_plan_set_shape_batch")

    def run(self, stream_ptr: int = 0) -> None:
        self._check(self.lib.rl_plan_run(self.h, C.c_void_p(stream_ptr) if stream_ptr else None), "rl_plan_run")

    @staticmethod
    def run_group(plans, stream_ptr: int = 0) -> None:
        hs = (C.c_void_p * len(plans))(*[pl.h.value for pl in plans])
        plans[0]._check(plans[0].lib.rl_plan_run_group(hs, len(plans), C.c_void_p(stream_ptr) if stream_ptr else None),
                        "rl_plan_run_group")

    def kernel_ms(self, idx: int) -> float:
        """HIP-event ms of the last run: idx 1 / 2 the mode's kernel, 0 the whole run (waits for it)."""
        ms = C.c_float()
        self._check(self.lib.rl_plan_kernel_ms(self.h, idx, C.byref(ms)), "rl_plan_kernel_ms")
        return float(ms.value)

    def fetch(self) -> dict:
        """mode -> abi.Outputs of the last run."""
        outs = {m: abi.Outputs.alloc(self.B, self.N, self.max_outer, m == MT) for m in (MC, MT) if self.modes & m}
        cs = {m: o.as_c() for m, o in outs.items()}
        self._check(self.lib.rl_plan_fetch(self.h, C.byref(cs[MC]) if MC in cs else None,
                                           C.byref(cs[MT]) if MT in cs else None), "rl_plan_fetch")
        return outs

    def close(self) -> int:
        rc = self.lib.rl_plan_destroy(self.h) if self.h else 0
        self.h = None
        return rc


@functools.lru_cache(maxsize=None)
def load(case: str, open_path: bool = False):
    """(problem, cfg) of a fixture; open_path: its rings as open polylines (bench.open_problem)."""
    c = O.load_case(case)
    prob = O.case_problem(c)
    if open_path:
        prob = abi.Problem(center=prob.center, L=prob.L, inner_seg=raceline.edges_for(c["inner_ring"], False),
                           outer_seg=raceline.edges_for(c["outer_ring"], False), veh_width=prob.veh_width, closed=False)
    return prob, O.case_cfg(c)


def make_plans(lib, wl: Workload, B: int, modes=None, seed0: int = 0) -> list:
    """The plans of a workload at batch size B on one library, in case order, then mode order."""
    modes = tuple(modes or wl.modes)
    plans = []
    try:
        for case in wl.cases:
            prob, cfg = load(case, wl.open)
            if wl.grid:             # the sweep's base cfg is the first track's (bench.run_c4)
                cfg = load(wl.cases[0], wl.open)[1]
            cfg = abi.RlCfg.from_dict({**cfg.to_dict(), **dict(wl.cfg)})
            for m in modes:
                pl = LibPlan(lib, prob, D.c4_cfgs(cfg)[:B] if wl.grid else cfg,
                             np.arange(seed0, seed0 + B, dtype=np.uint64) if wl.seeds else None, B, m, label=case)
                plans.append(pl)
                if wl.grid:         # concurrent plans take the shape of the whole load (bench.run_c4)
                    pl.set_shape_batch(len(wl.cases) * len(modes) * B)
    except Exception:
        close_plans(plans)
        raise
    return plans


def close_plans(plans) -> list:
    return [pl.close() for pl in plans]


def run_plans(plans, schedule: str = "each", streams=None) -> float:
    """One round of one library's plans; returns the wall ms until all have finished."""
    t0 = time.perf_counter()
    if schedule == "each":
        for pl in plans:
            pl.run()
            pl.kernel_ms(0)
    elif schedule == "streams":
        for pl, st in zip(plans, streams):
            pl.run(st.cuda_stream)
        for st in streams:
            st.synchronize()
    elif schedule == "group":
        LibPlan.run_group(plans, streams[0].cuda_stream)
        streams[0].synchronize()
    else:
        raise ValueError(f"schedule {schedule!r}: each, streams or group")
    return (time.perf_counter() - t0) * 1e3


def make_streams(n: int) -> list:
    import torch

    return [torch.cuda.Stream() for _ in range(n)]


def differing(a: dict, b: dict) -> list:
    """Names ("min-time.lap") of the FIELDS in which two fetch() results differ."""
    return [f"{MODE_NAME[m]}.{f}" for m in a for f in FIELDS[m] if not np.array_equal(getattr(a[m], f), getattr(b[m], f))]


def interleave(cases: dict, rounds: int, repeat: int = 1) -> dict:
    """name -> [last result of `repeat` calls in a row] over `rounds` rounds, the cases taking
    turns inside every round, after one unrecorded call of each."""
    for f in cases.values():
        f()
    res = {k: [] for k in cases}
    for _ in range(rounds):
        for k, f in cases.items():
            for _ in range(repeat):
                v = f()
            res[k].append(v)
    return res


def med_min_max(v) -> dict:
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def last_call_kernel_ms(lib) -> float:
    """The min-curvature kernel's ms of the last rl_optimize call (rl_last_call_times)."""
    run, k, call = C.c_float(), C.c_float(), C.c_float()
    lib.rl_last_call_times(C.byref(run), C.byref(k), None, C.byref(call))
    return k.value


# ------------------------------------------------------------------ timing
def time_workload(libs: dict, wl: Workload, B: int = None, modes=None, rounds: int = 4, schedule: str = None,
                  per_plan: bool = False, name: str = "", out=print) -> dict:
    """Time one workload at one batch size over `libs` (name -> path of a librl.so).

    Every (library, environment of wl.envs) pair is an entry.  All plans are created first;
    then `rounds` rounds run with the entries interleaved inside each round and the first round
    is dropped.  Returns entry -> {"ms": {column: [per kept round]}, "differs": [field names that
    differ from the first entry], "bitexact": bool, "destroy_rc": [rl_plan_destroy per plan]};
    the columns are min-curv / min-time (rl_plan_kernel_ms of the mode, summed over the plans),
    run (the run bracket, index 0) and, for the concurrent schedules, wall.  Plans are always
    destroyed."""
    if rounds < 2:
        raise ValueError("rounds >= 2: the first round is dropped")
    B = B or wl.B[0]
    schedule = schedule or wl.schedule
    entries = {}
    res = {}
    try:
        for n, path in libs.items():
            lib = load_library(path)
            for env in wl.envs:
                key = n + "".join(f"[{k}={v}]" for k, v in env) if len(wl.envs) > 1 else n
                with environ(env):
                    entries[key] = (env, make_plans(lib, wl, B, modes))
        first = next(iter(entries.values()))[1]
        streams = make_streams(len(first)) if schedule != "each" else None
        cols = [MODE_NAME[m] for m in (MC, MT) if any(pl.modes & m for pl in first)] + ["run"] + ["wall"] * (schedule != "each")
        ms = {k: {c: [] for c in cols} for k in entries}
        for r in range(rounds):
            for k, (env, plans) in entries.items():
                with environ(env):
                    wall = run_plans(plans, schedule, streams)
                if r == 0:
                    continue
                for m in (MC, MT):
                    if MODE_NAME[m] in cols:
                        ms[k][MODE_NAME[m]].append(sum(pl.kernel_ms(m) for pl in plans if pl.modes & m))
                ms[k]["run"].append(sum(pl.kernel_ms(0) for pl in plans))
                if schedule != "each":
                    ms[k]["wall"].append(wall)
        tag = f"{name.upper() or 'AB'} B={B} modes={'+'.join(map(str, modes or wl.modes))}"
        for k in entries:
            out(f"{tag} {k:12s} " + "  ".join(f"{c} median {np.median(v):8.2f} ms  min {min(v):8.2f}" for c, v in ms[k].items()))
        if per_plan:                # each plan alone, its kernel time (min of 3 runs)
            for k, (env, plans) in entries.items():
                per = []
                with environ(env):
                    for pl in plans:
                        best = 1e9
                        for _ in range(3):
                            pl.run()
                            best = min(best, pl.kernel_ms(0))
                        per.append(f"{pl.N}:{'+'.join('mc' if m == MC else 'mt' for m in (MC, MT) if pl.modes & m)}:{best:.2f}")
                out(f"per-plan kernel ms {k:10s} " + " ".join(per))
            for env, plans in entries.values():      # (the compare below reads the schedule's results)
                with environ(env):
                    run_plans(plans, schedule, streams)
        base_key, base = next(iter(entries)), None
        for k, (env, plans) in entries.items():
            got = [pl.fetch() for pl in plans]
            if base is None:
                base = got
            diff = sorted({f for a, b in zip(got, base) for f in differing(a, b)})
            evals = np.concatenate([o.evals.ravel() for g in got for o in g.values()])
            res[k] = {"ms": ms[k], "differs": diff, "bitexact": not diff}
            out(f"{tag} {k:12s} bitexact_vs_{base_key}: {not diff}; evals/outer {evals.mean():.2f}, {int(evals.sum())} evaluations")
            if diff:
                dmax = lambda f: max([float(np.max(np.abs(getattr(a[m], f) - getattr(b[m], f))))   # noqa: E731
                                      for a, b in zip(got, base) for m in a if getattr(a[m], f) is not None] or [0.0])
                out(f"    differs: {diff} max |dlap| {dmax('lap')} max |dx| {dmax('x')}")
    finally:
        for k, (env, plans) in entries.items():
            res.setdefault(k, {})["destroy_rc"] = close_plans(plans)
    return res


# ------------------------------------------------------------------ stamps and counters
# slot names of the RL_STAMPS builds, once per kernel family (16 slots of cycles per block)
_BODY = ["setup", "corridor tail (combine, LDS, seed)", "mt: kappa / v-pass / gamma", "lin-geom", "PGD loop", "update", "final",
         "normals + corridor loads", "corridor: inner-ring rays", "corridor: outer-ring rays", "corridor: fallback search"]
_NORMALS = ["normals + their barrier (slot 7: the scan's loads alone)"]
STAMP_SLOTS = {
    "reg": _BODY + _NORMALS,
    "mid": _BODY + _NORMALS,
    # VSPLIT (min-time, K = 1): slots 12-15 are other waves' cycles, or counted in 7-10 already
    "lat": _BODY + ["normals + their barrier / vsplit: join wait + collect (wave 0)", "vsplit: v-pass wave's v-pass [not in the sum]",
                    "vsplit: wave 0 scan [in 7-10]", "vsplit: wave 1 scan [not in the sum]", "vsplit: wave 2 scan [not in the sum]"],
    # RL_STAMPS_EVAL (variant stamps_eval): the evaluation's phases, slot 4 = the rest of the loop
    "eval": _BODY + ["pgd: projection", "pgd: stencil+partials", "pgd: wave sum", "pgd: barrier+block sum", "pgd: gradient"],
    "stream": ["setup", "corridor tail (write, seed)", "mt: gamma^2 (+ lap)", "lin-geom", "PGD loop", "update", "normals",
               "corridor loads", "corridor: inner-ring rays", "corridor: outer-ring rays", "corridor: fallback search",
               "v-pass: store", "v-pass: forward relaxations", "v-pass: backward relaxations", "v-pass: wraps, sweep checks",
               "v-pass: load kappa, v_kappa"],
}
STAMP_READ = {"reg": "rl_debug_stamps", "mid": "rl_debug_stamps_mid", "lat": "rl_debug_stamps_lat",
              "stream": "rl_debug_stamps_stream"}
COUNT_NAMES = ["ray blocks", "ray blocks visited", "ray walk iters (wave)", "exact ray tests (lane)",
               "md blocks", "md blocks visited", "md walk iters (wave)", "exact dists (lane)"]


def kernel_family(N: int, B: int, mode: int) -> tuple:
    """(family, K, T) of the kernel the library launches: stream, mid (4, 512), lat (the
    latency table's K <= 2 rows) or reg (rl_kernels.hip), by abi.kernel_shape."""
    K, T = abi.kernel_shape(N, B, mode)
    return ("stream" if K == 0 else "mid" if (K, T) == (4, 512) else "lat" if K <= 2 else "reg"), K, T


def stamps_workload(lib, wl: Workload, B: int = None, modes=None, seed0: int = 0, eval_slots: bool = False,
                    name: str = "", out=print) -> list:
    """Phase shares of every (case, mode, environment) of a workload from an RL_STAMPS build
    (shares only: a stamped build's time is not the real kernel's).  One single-mode plan at a
    time, two runs; returns [(case, mode, family, cycles[16])]."""
    B = B or wl.B[0]
    rows = []
    for case in wl.cases:
        for mode in (m for w in (modes or wl.modes) for m in (MC, MT) if w & m):
            for env in wl.envs:
                with environ(env):
                    fam, K, T = kernel_family(load(case, wl.open)[0].N, B, mode)
                    pl = make_plans(lib, replace(wl, cases=(case,)), B, (mode,), seed0)[0]
                    try:
                        pl.run()
                        pl.run()
                        ms = pl.kernel_ms(mode)
                        st = np.zeros((B, 16), dtype=np.uint64)
                        rc = getattr(lib, STAMP_READ[fam])(st.ctypes.data_as(C.c_void_p), B)
                        assert rc == 0, (STAMP_READ[fam], rc)
                        n_ev = int(pl.fetch()[mode].evals.sum())
                    finally:
                        pl.close()
                names = STAMP_SLOTS["eval" if eval_slots and fam != "stream" else fam]
                tot = st.sum(0).astype(float)
                own = tot.sum() - (tot[12:16].sum() if names is STAMP_SLOTS["lat"] else 0.0)     # wave 0's own cycles
                out(f"{name.upper()} {case} N={pl.N} mode={mode} B={B} seeds {seed0 if wl.seeds else None}.. "
                    f"{dict(env) or ''} shape=({K},{T}) kernel {ms:.2f} ms (stamped); per-block cycles {own / B:.3e}, "
                    f"{n_ev} evaluations ({own / max(n_ev, 1):.0f} cycles each, all phases)")
                for i, nm in enumerate(names):
                    if tot[i] > 0:
                        out(f"   {nm:44s} {100 * tot[i] / own:5.1f}%  {tot[i] / B:.3e} cyc/block")
                rows.append((case, mode, fam, tot))
    return rows


def counts_workload(lib, wl: Workload, B: int = 16, outers=(None,), first_seed: int = 0, name: str = "", out=print) -> dict:
    """Corridor work counters (RL_COUNT build) of a workload's min-curvature run, B seeds from
    first_seed, per max_outer_iters of `outers` (None: the cfg's).  Register-resident shapes
    are counted in C2's own shape (a batch of 16 alone would get a latency shape).  Returns
    max_outer -> [8 counters] of the last case."""
    res = {}
    for case in wl.cases:
        prob = load(case, wl.open)[0]
        for mo in outers:
            w = replace(wl, cases=(case,), cfg=wl.cfg + (() if mo is None else (("max_outer_iters", mo),)))
            with environ(wl.envs[0]):
                stream = kernel_family(prob.N, 1024, MC)[0] == "stream"
                pl = make_plans(lib, w, B, (MC,), first_seed)[0]
                try:
                    if not stream:
                        pl.set_shape_batch(1024)
                    dbg = lib.rl_debug_counts if stream else lib.rl_debug_counts_reg     # (the kernel's translation unit)
                    cnt = np.zeros(8, dtype=np.uint64)
                    dbg(cnt.ctypes.data_as(C.c_void_p), 1)
                    pl.run()
                    o = pl.fetch()[MC]
                    dbg(cnt.ctypes.data_as(C.c_void_p), 0)
                finally:
                    pl.close()
            passes = B * (pl.max_outer + 1) * prob.N
            out(f"{name.upper()} {case} N={prob.N} B={B} max_outer={pl.max_outer} rings {prob.inner_seg.shape[0]}+{prob.outer_seg.shape[0]}"
                f" evals/outer {o.evals.mean():.2f}")
            for nm, v in zip(COUNT_NAMES, cnt):
                out(f"   {nm:26s} {int(v):14d}  per sample-pass {v / passes:9.3f}")
            res[pl.max_outer] = [int(v) for v in cnt]
            out(json.dumps({"max_outer": pl.max_outer, "ray_blocks": res[pl.max_outer][0], "ray_blocks_visited": res[pl.max_outer][1],
                            "visited_fraction": round(res[pl.max_outer][1] / max(1, res[pl.max_outer][0]), 4)}))
    if 1 in res and len(res) > 1:       # the later passes alone (the most outer iterations minus the one pass of max_outer 1)
        last = res[max(res)]
        out(json.dumps({"first_pass_visited": round(res[1][1] / max(1, res[1][0]), 4),
                        "later_passes_visited": round((last[1] - res[1][1]) / max(1, last[0] - res[1][0]), 4)}))
    return res


def counts_corridor(lib, wl: Workload, name: str = "", out=print) -> None:
    """The same counters for rl_corridor (one pass, 2 adjacent samples per lane)."""
    for case in wl.cases:
        prob, cfg = load(case, wl.open)
        cnt = np.zeros(8, dtype=np.uint64)
        lib.rl_debug_counts_geom(cnt.ctypes.data_as(C.c_void_p), 1)
        lo, hi = np.zeros(prob.N), np.zeros(prob.N)
        p = prob.as_c()
        assert lib.rl_corridor(C.byref(p), C.byref(cfg), 0, abi.dptr(lo), abi.dptr(hi)) == 0
        lib.rl_debug_counts_geom(cnt.ctypes.data_as(C.c_void_p), 0)
        out(f"{name.upper()} rl_corridor {case} N={prob.N}")
        for nm, v in zip(COUNT_NAMES, cnt):
            out(f"   {nm:26s} {int(v):14d}  per sample {v / prob.N:9.3f}")


# ------------------------------------------------------------------ command line
def run_workload(lib, wl: Workload, B: int, modes, inners, launches: int, name: str = "", out=print) -> None:
    """A few launches of one library's plans and nothing else: the command a profiler wraps.
    One block of launches per max_inner_iters of `inners` (None: the cfg's); the last line is
    the JSON scripts/pmc_split_report.py reads."""
    evals = []
    for inner in inners:
        w = wl if inner is None else replace(wl, cfg=wl.cfg + (("max_inner_iters", inner),))
        with environ(w.envs[0]):
            plans = make_plans(lib, w, B, modes)
            try:
                for _ in range(launches):
                    run_plans(plans, "each")
                    out(f"{name.upper()} max_inner_iters={plans[0]._keep[1][0].max_inner_iters}: kernel " +
                        " ".join(f"{pl.kernel_ms(0):.3f}" for pl in plans) + " ms")
                ev = np.concatenate([o.evals.ravel() for pl in plans for o in pl.fetch().values()])
                out(f"evals/outer {ev.mean():.2f}")
                evals.append(int(ev.sum()))
                fam, K, T = kernel_family(plans[0].N, B, MT if plans[0].modes == MT else MC)
            finally:
                close_plans(plans)
    out(json.dumps({"evals": evals, "waves": B * T // 64}))


def list_tables(out=print) -> None:
    out("workloads:")
    for n, w in WORKLOADS.items():
        out(f"  {n:6s} B={','.join(map(str, w.B)):9s} modes={w.modes} {w.schedule:8s} {w.what}"
            + "".join(f" [{k}={v}]" for e in w.envs for k, v in e))
    out("variants (scripts/build_variants.py):")
    for n, d in VARIANTS.items():
        out(f"  {n:14s} {d}")


def _ints(s: str, default=None) -> list:
    return [default if x == "default" else int(x) for x in s.split(",")]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--list", action="store_true", help="print the workloads and the variants; needs no GPU")
    ap.add_argument("command", nargs="?", choices=("time", "run", "stamps", "counts"))
    ap.add_argument("workloads", nargs="?", default=os.environ.get("AB_CASES"),
                    help="comma-separated names of WORKLOADS, or all (default: AB_CASES)")
    ap.add_argument("--variants", default=None, help="patterns of _lib/variants/librl_<pattern>.so; product: the product library")
    ap.add_argument("--variant", default="stamps", help="stamps: the diagnostic build to read (stamps, stamps_eval)")
    ap.add_argument("--B", type=int, default=None)
    ap.add_argument("--modes", "--mode", type=int, default={"mc": MC, "mt": MT}.get(os.environ.get("AB_MODE", "")),
                    help="1 min-curv, 2 min-time, 3 both in one plan (AB_MODE=mc|mt)")
    ap.add_argument("--rounds", type=int, default=4, help="interleaved rounds, the first one dropped")
    ap.add_argument("--schedule", choices=("each", "streams", "group"), default=None)
    ap.add_argument("--per-plan", action="store_true", default=bool(os.environ.get("AB_PER_PLAN")))
    ap.add_argument("--env", default=None, help="NAME=v0,v1: run every library under each value, interleaved")
    ap.add_argument("--inner", default=os.environ.get("INNER"), help="max_inner_iters (run: a list, `default` = the cfg's)")
    ap.add_argument("--launches", type=int, default=2)
    ap.add_argument("--seed0", type=int, default=0)
    ap.add_argument("--outer", default=None, help="counts: max_outer_iters values, e.g. 1,2,14")
    ap.add_argument("--corridor", action="store_true", help="counts: rl_corridor's counters too")
    a = ap.parse_args(argv)
    if a.list:
        list_tables()
        return 0
    if not a.command or not a.workloads:
        ap.error("a command and a workload (or --list)")
    names = list(WORKLOADS) if a.workloads == "all" else a.workloads.split(",")
    if set(names) - set(WORKLOADS):
        ap.error(f"unknown workload {sorted(set(names) - set(WORKLOADS))}; known: {', '.join(WORKLOADS)}")
    modes = (a.modes,) if a.modes else None
    for n in names:
        wl = WORKLOADS[n]
        cases = os.environ.get({"stamps": "ST_CASES", "counts": "COUNT_CASE"}.get(a.command, ""))
        if cases:                   # the fixtures to read out instead of the workload's own
            wl = replace(wl, cases=tuple(cases.split(",")))
        if a.env:
            k, vals = a.env.split("=", 1)
            wl = replace(wl, envs=tuple(e + ((k, v),) for e in wl.envs for v in vals.split(",")))
        if a.command == "time":
            if a.inner is not None:
                wl = replace(wl, cfg=wl.cfg + (("max_inner_iters", int(a.inner)),))
            libs = find_libs(a.variants or "*")
            for B in ([a.B] if a.B else wl.B):
                time_workload(libs, wl, B, modes, a.rounds, a.schedule, a.per_plan, n)
            if (a.schedule or wl.schedule) != "each":
                print(f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}")
        elif a.command == "run":
            lib = load_library(next(iter(find_libs(a.variants or "product").values())))
            run_workload(lib, wl, a.B or wl.B[0], modes, _ints(a.inner or "default"), a.launches, n)
        elif a.command == "stamps":
            stamps_workload(load_library(variant_path(a.variant)), wl, a.B, modes, a.seed0, a.variant == "stamps_eval", n)
        else:
            lib = load_library(variant_path("count"))
            wl = replace(wl, envs=tuple(e + (("RL_FORCE_STREAM", "1"),) for e in wl.envs)) if not a.outer else \
                replace(wl, envs=tuple(e + (("RL_CORRIDOR0", os.environ.get("RL_CORRIDOR0", "0")),) for e in wl.envs))
            counts_workload(lib, wl, a.B or 16, _ints(a.outer) if a.outer else (None,), 1 if a.outer else 0, n)
            if a.corridor:
                counts_corridor(lib, wl, n)
    return 0


if __name__ == "__main__":
    sys.exit(main())
