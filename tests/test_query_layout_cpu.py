"""The packed blocks of the pose-query stages (csrc/rl_query.h), checked without a GPU.

tests/query_layout_check.cpp is a stand-alone program (its own main, no HIP call); here it checks
the horizon (K = 0) and rejoin layouts of its shapes: the byte counts against their closed forms,
every byte of the queries' block with row and seg_hint given and NULL, the launch pointers written
through over a buffer of exactly out_bytes between two guard lines, and the copies into rl_hzn /
rl_rjn with every field, with alternating fields NULL and (rejoin) from the head alone.
tests/layout_check.py builds and runs it: with AddressSanitizer and UBSan on the host side where
that links, without them otherwise, and the test says which.

tests/golden/query_layout/offsets.json is the record of where every array of every stage lay
before the layouts were generated from one table (printed by a program of the same form compiled
against that header): the program's "dump" must equal it entry for entry, so no byte of either
block has moved.
"""
import json
import os

import pytest

import layout_check as LC

GOLDEN = os.path.join(LC.REPO, "tests", "golden", "query_layout", "offsets.json")


def test_query_layout(tmp_path):
    if not os.path.exists(LC.HIPCC):
        pytest.skip("hipcc not available")
    assert "horizon layout ok" in LC.run_stage(tmp_path, "horizon")
    assert "rejoin layout ok" in LC.run_stage(tmp_path, "rejoin")


def test_query_layout_offsets_are_the_recorded_ones(tmp_path):
    if not os.path.exists(LC.HIPCC):
        pytest.fail(f"{LC.HIPCC} is missing: the layout check cannot be built (the library's build needs it too)")
    got = json.loads(LC.run_stage(tmp_path, "dump"))
    want = json.load(open(GOLDEN))
    assert got["slots"] == want["slots"]
    assert len(got["layouts"]) == len(want["layouts"]) == 56
    for g, w in zip(got["layouts"], want["layouts"]):
        key = {k: w[k] for k in ("kind", "Q", "M", "K", "C")}
        assert {k: g[k] for k in key} == key
        for k in ("in_bytes", "head_bytes", "out_bytes", "scratch_bytes"):
            assert g[k] == w[k], (key, k)
        moved = [(n, a, b) for n, a, b in zip(want["slots"], g["off"], w["off"]) if a != b]
        assert not moved, (key, moved)
