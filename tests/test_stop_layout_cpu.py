"""The packed blocks of the stop stage (csrc/rl_query.h with `stop` set), checked without a GPU.

tests/query_layout_check.cpp is a stand-alone program (its own main, no HIP call); run as "stop" it
checks the stop layouts of its shapes: the byte counts against their
closed forms, the rejoin part of the queries' block at the rejoin stage's offsets, every byte of
the queries' block with v_target given and NULL, the launch pointers written through over a
buffer of exactly out_bytes between two guard lines, and the copies into rl_stp with every field,
with alternating fields NULL, from the head alone and with node_b alone.  tests/layout_check.py
builds and runs it, as for test_query_layout_cpu.py: with AddressSanitizer and UBSan on the host
side, and run directly; where that build does not link, it is built without them and the test
says so.
"""
import os

import pytest

import layout_check as LC


def test_stop_layout(tmp_path):
    if not os.path.exists(LC.HIPCC):
        pytest.fail(f"{LC.HIPCC} is missing: the layout check cannot be built (the library's build needs it too)")
    assert "stop layout ok" in LC.run_stage(tmp_path, "stop")
