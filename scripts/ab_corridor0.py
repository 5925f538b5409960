#!/usr/bin/env python3
"""A/B of the batch-wide first corridor (KParams::lo0/hi0, rl_plan_run): the same plans run
with RL_CORRIDOR0=1 (outer iteration 0's corridor cast once per batch by rl_corridor_kernel)
and RL_CORRIDOR0=0 (every instance casts it), interleaved by scripts/ab.py's timing function
(the product library under two environments); kernel ms of the mode's own events plus the
run bracket, and the outputs compared bit for bit.
usage: python scripts/ab_corridor0.py [rounds]    (AB_CASES=C2,C5 selects)"""
import json
import os
import sys
from dataclasses import replace

import numpy as np

import ab
from practice_path_planning_for_formula_student_driverless_amd import abi

W = ab.WORKLOADS
CASES = {"C2": (W["c2"], 1024, ab.MC), "C3mt": (W["c3mt"], 4096, ab.MT), "C5": (W["c5"], 1024, ab.MC),
         "C5mt": (W["c5mt"], 1024, ab.MT), "C4t3": (W["c4t3"], 512, ab.MT),
         "C4tm": (replace(W["c4t3"], cases=("track_training_map",)), 512, ab.MC)}
ON, OFF = "product[RL_CORRIDOR0=1]", "product[RL_CORRIDOR0=0]"

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sel = os.environ.get("AB_CASES")
for name, (wl, B, mode) in CASES.items():
    if sel and name not in sel.split(","):
        continue
    wl = replace(wl, envs=((("RL_CORRIDOR0", "1"),), (("RL_CORRIDOR0", "0"),)))
    r = ab.time_workload({"product": abi.LIB_PATH}, wl, B, (mode,), rounds + 1, name=name, out=lambda s: None)
    med = lambda k, c: round(float(np.median(r[k]["ms"][c])), 3)   # noqa: E731
    print(json.dumps({name: {"bitexact": r[OFF]["bitexact"], "on_kernel_ms": med(ON, ab.MODE_NAME[mode]),
                             "off_kernel_ms": med(OFF, ab.MODE_NAME[mode]), "on_run_ms": med(ON, "run"),
                             "off_run_ms": med(OFF, "run")}}), flush=True)
