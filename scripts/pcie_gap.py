"""Why is C2's kernel slower inside rl_optimize (host buffers, the drop-in path) than in the
device-resident plan the bench times?  The same C2 launch (B=1024, min-curv), the optimiser
kernel alone from its own HIP events:
  plan_b2b     rl_plan_run back to back, no host work between launches
  plan_sleep   rl_plan_run with a 3.5 ms host sleep between launches (the time rl_optimize
               spends copying results into the caller's buffers)
  plan_spin    the same gap spent busy-waiting on the host
  plan_copy    rl_plan_run + rl_plan_fetch into fresh host arrays each time
  optimize     rl_optimize (plan cache hit, pinned staging, threaded host copies)
  gap sweep    kernel ms against the GPU idle gap before each launch (0 .. 4 ms of host spin,
               interleaved): the drop-in call pays the gapped figure
Run under rocprofv3 --kernel-trace the kernel durations can be read per launch too.
usage: python scripts/pcie_gap.py [reps]"""
import json
import sys
import time

import numpy as np

import ab
from practice_path_planning_for_formula_student_driverless_amd import abi, raceline

lib = ab.load_library()
prob, cfg = ab.load("cmap1_n2000")
B = 1024
seeds = np.arange(B, dtype=np.uint64)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
plan = ab.make_plans(lib, ab.WORKLOADS["c2"], B)[0]
plan.run()
plan.kernel_ms(1)


def spin(s):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < s:
        pass


def after(gap):
    def f():
        plan.run()
        k = plan.kernel_ms(1)      # waits for the run
        gap()
        return k
    return f


def before(ms):
    def f():
        spin(ms * 1e-3)
        plan.run()
        return plan.kernel_ms(1)
    return f


res = {k: [after(g)() for _ in range(reps)] for k, g in (
    ("plan_b2b", lambda: None), ("plan_sleep", lambda: time.sleep(0.0035)), ("plan_spin", lambda: spin(0.0035)),
    ("plan_copy", plan.fetch))}
gaps = ab.interleave({str(g): before(g) for g in (0.0, 0.05, 0.2, 0.5, 1.0, 2.0, 4.0)}, reps)
plan.close()
raceline.optimize_batch(prob, cfg, seeds, B, mintime=False)
ms, calls = [], []
for _ in range(reps):
    t0 = time.perf_counter()
    out = raceline.optimize_batch(prob, cfg, seeds, B, mintime=False)
    calls.append(1e3 * (time.perf_counter() - t0))
    del out
    ms.append(ab.last_call_kernel_ms(lib))
res["optimize"] = ms
res["optimize_call_ms"] = calls
print(json.dumps({k: [round(x, 3) for x in v] for k, v in res.items()}))
print(json.dumps({k: round(float(np.median(v)), 3) for k, v in res.items()}), flush=True)
print(json.dumps({"kernel_ms_by_gap_ms": {g: ab.med_min_max(v)["median"] for g, v in gaps.items()},
                  "min": {g: ab.med_min_max(v)["min"] for g, v in gaps.items()}}), flush=True)
