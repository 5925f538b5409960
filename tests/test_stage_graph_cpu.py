"""csrc/rl_stage_graph.h, the table of a plan's run and stages, without a device:
tests/stage_graph_check.cpp holds, written out, what enqueuing each of the thirteen invalidates, the
stage of every rl_plan_kernel_ms index as include/rl_abi.h lists them, and the stage <-> QueryKind
mapping, and checks the header against them.  Built and run as tests/layout_check.py builds the
layout program."""
import os

import layout_check


def test_stage_graph_matches_the_written_out_tables(tmp_path):
    out = layout_check.run_stage(tmp_path, "all", os.path.join(layout_check.REPO, "tests", "stage_graph_check.cpp"))
    assert "stage graph: all checks passed" in out and "FAIL" not in out
    assert out.count(" clears 0x") == 13
