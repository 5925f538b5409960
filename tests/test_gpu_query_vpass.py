"""The rejoin and the stop kernel (rl_rejoin.hip, rl_stop.hip through rl_rejoin and rl_stop) against
the CPU oracle's v-pass, directly and bit for bit (DESIGN §3m, §3n "Anchored to the oracle"), not
through raceline.rejoin_host / raceline.stop_host: a reading of the reference's ax_max_at that
the kernels and those specifications shared would fail here.  The rows, the node ranges and the
bit view are those of tests/test_query_vpass_cpu.py (vpass_anchor_cases); one launch per stage
and cfg, B = Q = 3 rows of N = 300.  Nothing gets a tolerance.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before librl.so is loaded: torch then initialises its own HIP runtime first)

import cfg_cases
import query_cases as QC
import vpass_anchor_cases as VA
from practice_path_planning_for_formula_student_driverless_amd import abi, raceline
from vpass_anchor_cases import B, N

pytestmark = pytest.mark.gpu

KW = dict(dt=0.05, m_cap=8, k_cap=1024)


def _lib():
    return QC.lib(abi.RL_FEATURE_REJOIN | abi.RL_FEATURE_STOP)


def _stop(case, **kw):
    a = VA.anchor(case, True)
    return raceline.stop(*a.rows, a.h, False, cfg=cfg_cases.case_cfg(case), **VA.stop_query(a), **{**KW, **kw}), a


@pytest.mark.parametrize("case", VA.CASES)
def test_stop_kernel_march_and_envelope_are_the_oracles_vpass(case):
    _lib()
    got, a = _stop(case)
    assert got.node_v.shape == got.node_b.shape == (B, KW["k_cap"] + 1)
    phases = VA.check_stop(got, a, case, "rl_stop")
    print(f"{case}: (acceleration, plateau, brake) nodes {phases}")
    if case == "default":
        assert all(min(p) >= 10 for p in phases.values()), phases


@pytest.mark.parametrize("case", VA.CASES)
def test_rejoin_kernel_march_is_the_oracles_vpass_up_to_the_merge(case):
    _lib()
    a = VA.anchor(case, False)
    got = raceline.rejoin(*a.rows, a.h, False, a.poses, a.v0, cfg_cases.case_cfg(case), row=a.row, **KW)
    ends = VA.check_rejoin(got, a, case, "rl_rejoin")
    print(f"{case}: merge_node {got.merge_node.tolist()}, compared up to {ends}")
    # the one exclusion (VA.EXCLUDED states the reason): the other rows stand in for it
    assert set(VA.ROWS) - set(ends) == ({"wave"} if case == "vcap_huge" else set())
    assert ends["flat"] >= 10 and ends["tight_h02"] >= 10
    assert np.all(got.overspeed == 0)


@pytest.mark.parametrize("case", ["default", "caps_small"])
def test_k_cap_equal_to_the_last_node(case):
    """K_cap = N - 1: the stop's target, and the rejoin march's row end, is the last node the
    march may take, and the node arrays have no column behind it.  (caps_small: the rejoin
    march never merges and takes every node.)"""
    _lib()
    got, a = _stop(case, k_cap=N - 1)
    assert got.node_v.shape == (B, N)
    VA.check_stop(got, a, case, "rl_stop k_cap = K")
    a = VA.anchor(case, False)
    got = raceline.rejoin(*a.rows, a.h, False, a.poses, a.v0, cfg_cases.case_cfg(case), row=a.row, dt=0.05, m_cap=8,
                          k_cap=N - 1)
    assert got.node_v.shape == (B, N)
    VA.check_rejoin(got, a, case, "rl_rejoin k_cap = K")
