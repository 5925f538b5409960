"""Build A/B variant libraries into _lib/variants/ (experiments only)."""
import os, sys
from concurrent.futures import ThreadPoolExecutor
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from practice_path_planning_for_formula_student_driverless_amd import build as B
VARIANTS = {
    "base": {},
    "k4t512w2": {"RL_MID_K": 4, "RL_MID_T": 512, "RL_MID_W": 2},
    "k4t512w4": {"RL_MID_K": 4, "RL_MID_T": 512, "RL_MID_W": 4},
    "ck4": {"RL_CK": 4},
    "mt_k8t256": {"RL_MIDMT_K": 8, "RL_MIDMT_T": 256},
    "old_w": {"RL_SMALLMT_W": 4, "RL_SMALL_W": 4, "RL_S8MT_W": 2},   # before the per-mode occupancy A/B
    "smc_w4": {"RL_SMALL_W": 4},
    "smc_w3": {"RL_SMALL_W": 3},
    "smt_w3": {"RL_SMALLMT_W": 3},
    "s8mt_w2": {"RL_S8MT_W": 2},
    "bt1": {"RL_BT_BATCH": 1},
    "bt6": {"RL_BT_BATCH": 6},
    "bt8": {"RL_BT_BATCH": 8},
    "sck1": {"RL_SCK": 1},
    "sck4": {"RL_SCK": 4},
    "ck1": {"RL_CK": 1},
    "blk8": {"RL_BLKSZ": 8},
    "blk32": {"RL_BLKSZ": 32},
    # scheduler A/B (build.py TU_FLAGS holds the product's choice; "_tu" overrides per source)
    "lat_default": {"_tu": {"csrc/rl_kernels_lat.hip": []}},
    "mid_default": {"_tu": {"csrc/rl_kernels_mid.hip": []}},
    "mid_ilp": {"_tu": {"csrc/rl_kernels_mid.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]}},
    "lat_iilp": {"_tu": {"csrc/rl_kernels_lat.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]}},
    "thr_ilp": {"_tu": {"csrc/rl_kernels.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]}},
    "thr_minreg": {"_tu": {"csrc/rl_kernels.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-minreg"]}},
    "thr_memclause": {"_tu": {"csrc/rl_kernels.hip": ["-mllvm", "-amdgpu-sched-strategy=max-memory-clause"]}},
    "thr_default": {"_tu": {"csrc/rl_kernels.hip": []}},
    "thr_bias0": {"_tu": {"csrc/rl_kernels.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-maxocc", "-mllvm", "-amdgpu-schedule-metric-bias=0"]}},
    "thr_trackers": {"_tu": {"csrc/rl_kernels.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-maxocc", "-mllvm", "-amdgpu-use-amdgpu-trackers"]}},
    "thr_def_bias0": {"_tu": {"csrc/rl_kernels.hip": ["-mllvm", "-amdgpu-schedule-metric-bias=0"]}},
    "stream_bias0": {"_tu": {"csrc/rl_stream.hip": ["-mllvm", "-amdgpu-schedule-metric-bias=0"]}},
    "stream_maxocc": {"_tu": {"csrc/rl_stream.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-maxocc"]}},
    # (iterative-ilp on rl_kernels.hip crashes this LLVM's register allocator on <8,256,closed,mintime>)
    "stream_iilp": {"_tu": {"csrc/rl_stream.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]}},
    "prio": {"RL_PRIO": 1},              # wave priority falling with the outer iteration (tail balance)
    "prio2": {"RL_PRIO": 2},             # the same with two levels
    "prio3": {"RL_PRIO": 3, "_tu": {"csrc/rl_kernels.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-maxocc"],
                                    "csrc/rl_kernels_group.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-maxocc"]}},   # end-weighted levels
    "prio_s": {"RL_PRIO": 1, "RL_SPRIO": 1},   # and in the streaming kernel
    "stamps": {"RL_STAMPS": 1},          # diagnostic (scripts/ab.py stamps); not A/B-timed
    "stamps_eval": {"RL_STAMPS": 1, "RL_STAMPS_EVAL": 1},   # + the latency evaluation's phases (scripts/ab.py stamps lat --variant stamps_eval)
    "count": {"RL_COUNT": 1},            # diagnostic (scripts/ab.py counts); not A/B-timed
}
if __name__ == "__main__":
    # usage: build_variants.py [NAME | ALIAS=NAME ...]   (ALIAS=NAME: the variant NAME built as librl_ALIAS.so)
    names = sys.argv[1:] or [n for n in VARIANTS if n not in ("stamps", "stamps_eval", "count")]
    jobs = [(a.split("=")[0], a.split("=")[-1]) for a in names]
    for _, name in jobs:
        if name not in VARIANTS:
            sys.exit(f"build_variants.py: no variant {name!r}; known: {', '.join(VARIANTS)}")
    import shutil; shutil.rmtree(os.path.join(B.LIB_DIR, "variants"), ignore_errors=True)
    with ThreadPoolExecutor(4) as ex:
        for p in ex.map(lambda j: B.build_variant(j[0], VARIANTS[j[1]]), jobs):
            print("built", p)
