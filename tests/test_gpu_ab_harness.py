"""The A/B harness (scripts/ab.py) on the GPU: the product library under two names must
report equal outputs, finite positive times, and leave no plan behind."""
import ctypes as C
import math
import os
import sys
from dataclasses import replace

import pytest

import oracle_lib as O
from practice_path_planning_for_formula_student_driverless_amd import abi

sys.path.insert(0, os.path.join(O.REPO, "scripts"))
import ab  # noqa: E402

pytestmark = pytest.mark.gpu


def _cache_info(lib):
    n, a, b = C.c_int32(), C.c_int64(), C.c_int64()
    assert lib.rl_plan_cache_info(C.byref(n), C.byref(a), C.byref(b)) == 0
    return n.value, a.value, b.value


# the smallest workloads that take each path: a register-resident kernel with both modes in one
# plan, and the streaming kernel
@pytest.mark.parametrize("wl, columns", [
    (replace(ab.WORKLOADS["c4t3"], cases=("track_training_map",)), ("min-curv", "min-time", "run")),
    (ab.WORKLOADS["c5"], ("min-curv", "run")),
], ids=["training_map_both_modes", "oval_n10000_mincurv"])
def test_same_library_under_two_names(wl, columns):
    lib = ab.load_library()
    before = _cache_info(lib)
    lines = []
    res = ab.time_workload({"a": abi.LIB_PATH, "b": abi.LIB_PATH}, wl, B=2, rounds=2, name="t", out=lines.append)
    assert list(res) == ["a", "b"]
    for name, r in res.items():
        assert r["bitexact"] and r["differs"] == [], (name, r["differs"])
        assert tuple(r["ms"]) == columns
        for col, v in r["ms"].items():
            assert len(v) == 1, (name, col, v)          # 2 rounds, the first dropped
            assert all(math.isfinite(x) and x > 0 for x in v), (name, col, v)
        assert r["destroy_rc"] == [0] * len(wl.cases) * len(wl.modes), name
    assert sum("bitexact_vs_a: True" in s for s in lines) == 2, lines
    assert _cache_info(lib) == before
