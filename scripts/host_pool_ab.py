#!/usr/bin/env python3
"""A/B of the host pool (abi.HostPool) in the drop-in call pattern: C2 (B=1024, min-curv)
through raceline.optimize_batch with fresh output arrays dropped after each call, pool on
and pool off, and into reused outputs; interleaved rounds, call ms (wall) and kernel ms
(the library's own HIP events), medians.  One pooled call after the rounds is compared with
the reused-output call bit for bit (a compare between timed calls would idle the GPU).
usage: python scripts/host_pool_ab.py [rounds]"""
import json
import os
import sys
import time

import numpy as np

import ab
from practice_path_planning_for_formula_student_driverless_amd import abi, raceline


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    lib = ab.load_library()
    prob, cfg = ab.load("cmap1_n2000")
    B = 1024
    seeds = np.arange(B, dtype=np.uint64)
    pool = abi.HOST_POOL
    cap = pool.cap
    keep = raceline.optimize_batch(prob, cfg, seeds, B, mintime=False)

    kms = lambda: ab.last_call_kernel_ms(lib)   # noqa: E731

    same = [True]

    def pooled(check=False):
        pool.cap = cap
        t0 = time.perf_counter()
        o = raceline.optimize_batch(prob, cfg, seeds, B, mintime=False)
        t = time.perf_counter() - t0
        if check:                # (only outside the timed rounds: the compare is a long host gap)
            same[0] &= all(np.array_equal(getattr(o[0], f), getattr(keep[0], f)) for f in abi.OUT_F64 + ("evals", "accepts"))
        del o
        return t * 1e3, kms()

    def no_pool():
        pool.cap = 0             # (new arrays plain numpy; the pool's free buffers stay for the next pooled call)
        t0 = time.perf_counter()
        o = raceline.optimize_batch(prob, cfg, seeds, B, mintime=False)
        t = time.perf_counter() - t0
        del o
        pool.cap = cap
        return t * 1e3, kms()

    def reused():
        t0 = time.perf_counter()
        raceline.optimize_batch(prob, cfg, seeds, B, mintime=False, out=keep)
        return (time.perf_counter() - t0) * 1e3, kms()

    # two calls per case: the second follows one of its own kind
    res = ab.interleave({"pool": pooled, "no_pool": no_pool, "reused": reused}, rounds, repeat=2)
    pooled(check=True)
    out = {k: {"call_ms": round(float(np.median([c for c, _ in v])), 3),
               "kernel_ms": round(float(np.median([k_ for _, k_ in v])), 3),
               "call_ms_min": round(float(np.min([c for c, _ in v])), 3)} for k, v in res.items()}
    out["pool_bitexact_vs_reused"] = bool(same[0])
    out["pool_hits"], out["pool_misses"] = pool.hits, pool.misses
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
