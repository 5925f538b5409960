#!/usr/bin/env python3
"""C4 as the bench runs it (7 bundled tracks x 512 sweep points x 2 modes = 14 single-mode
plans, shape batch 7168) under two schedules, interleaved rounds, wall ms of the whole sweep:
  s14    every plan on its own HIP stream (bench.run_c4 before rl_plan_run_group)
  group  rl_plan_run_group over the 14 plans: per mode one launch per K (the ragged form
         for a launch with any N % K != 0; profiles/r06/c4_group.log also holds the earlier
         split by N % K as `group` against this merged form as `group_mix`, and the merged
         form in plan order as `group` against longest-first as `group_sorted`, now the default)
and a bit-for-bit check of every plan's outputs (ab.FIELDS) between the two.
usage: python scripts/c4_group.py [rounds]   (GPU_MAX_HW_QUEUES as the environment sets it)"""
import os
import sys
import time

import numpy as np

import ab

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
plans = ab.make_plans(ab.load_library(), ab.WORKLOADS["c4"], 512)
streams = ab.make_streams(len(plans))
main = ab.make_streams(1)
scheds = {"s14": lambda: ab.run_plans(plans, "streams", streams), "group": lambda: ab.run_plans(plans, "group", main)}

scheds["s14"]()
ref = [pl.fetch() for pl in plans]
scheds["group"]()
same = {"group": not any(ab.differing(g, r) for g, r in zip([pl.fetch() for pl in plans], ref))}
res = {"s14": [], "group": []}
for _ in range(rounds):
    for name, f in scheds.items():
        res[name].append(f())
print(f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}; bit-exact vs s14: {same}")
for k, v in res.items():
    print(f"C4 {k:6s} wall ms: median {np.median(v):7.2f} min {np.min(v):7.2f}", flush=True)
ab.close_plans(plans)
