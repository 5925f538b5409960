#!/usr/bin/env python3
"""C4 schedules over the product library (no oracle; scripts/ab.py's c4 workload: 7 bundled
tracks x 512 sweep points x 2 modes), each timed in interleaved rounds, wall ms of the sweep:
  s14      the 14 single-mode plans, each on its own stream, in track order
  lptS     S streams, the plans sorted by their own measured time (longest first) and dealt
           to the least-loaded stream (longest-processing-time first); S = 2, 4, 7, 8 and
           GPU_MAX_HW_QUEUES
  both7    one plan per track with both modes (min-time on the plan's second stream), 7 streams
  mc->mt   all min-curv plans on 7 streams, join, then all min-time plans; mt->mc the reverse
(scripts/c4_group.py compares s14 with rl_plan_run_group, the bench's schedule.)
usage: python scripts/c4_schedules.py [rounds]"""
import os
import sys
import time

import numpy as np

import ab

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
lib = ab.load_library()
plans = ab.make_plans(lib, ab.WORKLOADS["c4"], 512)
both = ab.make_plans(lib, ab.WORKLOADS["c4"], 512, (ab.MC | ab.MT,))
mc, mt = plans[0::2], plans[1::2]
alone = []
for pl in plans:            # each plan alone (min of 3 runs)
    alone.append(min(ab.run_plans([pl]) for _ in range(3)))
order = sorted(range(len(plans)), key=lambda i: -alone[i])


def lpt(S):
    load, assign = [0.0] * S, [[] for _ in range(S)]
    for i in order:
        s = min(range(S), key=lambda j: load[j])
        assign[s].append(plans[i])
        load[s] += alone[i]
    return assign


def run_lists(lists, streams):
    for pls, st in zip(lists, streams):
        for pl in pls:
            pl.run(st.cuda_stream)
    for st in streams:
        st.synchronize()


st14 = ab.make_streams(14)
scheds = {"s14": lambda: run_lists([[pl] for pl in plans], st14), "both7": lambda: run_lists([[pl] for pl in both], st14),
          "mc->mt": lambda: (run_lists([[pl] for pl in mc], st14), run_lists([[pl] for pl in mt], st14)),
          "mt->mc": lambda: (run_lists([[pl] for pl in mt], st14), run_lists([[pl] for pl in mc], st14))}
for S in sorted({2, 4, 7, 8, int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))}):
    scheds[f"lpt{S}"] = (lambda lists, sts: lambda: run_lists(lists, sts))(lpt(S), ab.make_streams(S))


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


res = ab.interleave({k: (lambda f: lambda: timed(f))(f) for k, f in scheds.items()}, rounds)
print(f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}; plans alone (ms): " + " ".join(f"{a:.2f}" for a in alone))
for k, v in res.items():
    print(f"C4 schedule {k:6s} wall ms: median {np.median(v):7.2f} min {min(v):7.2f}", flush=True)
scheds["s14"]()
ref = [pl.fetch() for pl in plans]
scheds["both7"]()
got = [b.fetch() for b in both]
print("both7 outputs equal s14's:", not any(ab.differing({m: g[m]}, r) for g, rs in zip(got, zip(ref[0::2], ref[1::2])) for r in rs for m in r))
ab.close_plans(plans + both)
