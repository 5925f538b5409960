"""`fsd_raceline` with every stage switch in one invocation: the files and the stderr lines are those
of the stages run one by one.  The stages share the winners, the tick writer, the query filler and
std::cerr's formatting state; a buffer or a precision that leaked from one stage into the next
would show here and in no single-stage test."""
import math
import os
import shutil
import subprocess

import pytest

import test_host_cli as H

pytestmark = pytest.mark.gpu
ARGS = ["--seeds", "16", "--best", "2", "--mode", "mintime", "--trajectory-dt", "0.05", "--trajectory-cap", "2048"]
INPUTS = ("t_centerline.csv", "t_centerline_inner_from_mids.csv", "t_centerline_outer_from_mids.csv",
          "t_centerline_with_geom.csv")
TAGS = ("[rejoin]", "[stop]", "[retime]", "[recover-fan]", "[recover]", "[best]")


def _stage_run(src, d, extra):
    """ARGS + extra on a copy of the step-6 files in the fresh directory d: (stderr's stage lines, the new files)."""
    os.makedirs(d)
    for f in INPUTS:
        shutil.copy(src / f, d / f)
    r = subprocess.run([H._exe(), str(d / "t_centerline.csv"), *ARGS, *extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode == 0, (extra, r.stderr)
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith(TAGS)]
    return lines, {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f not in INPUTS}


def test_all_stages_in_one_invocation_equal_the_stages_alone(tmp_path):
    src = tmp_path / "steps"
    os.makedirs(src)
    r, _ = H._run("training_map", src)
    assert r.returncode == 0, r.stderr
    rejoin = ["--start-speed", "0"]
    stop = ["--stop-sample", "150", "--stop-speed", "3", "--stop-from", "60"]
    retime = ["--retime-set", "mu=0.8", "--retime-set", "a_lat_max=7.5", "--retime-from", "40"]
    alone = {"rejoin": _stage_run(src, tmp_path / "rejoin", rejoin)}
    # a car 0.4 m left of winner 0 at its sample 30, heading 10 degrees off the raceline's direction
    best0 = [tuple(map(float, ln.split(","))) for ln in alone["rejoin"][1]["t_centerline_best0_raceline.csv"].decode().splitlines()]
    (x0, y0), (x1, y1) = best0[30], best0[31]
    psi = math.atan2(y1 - y0, x1 - x0)
    car = ["--recover-from", f"{x0 - 0.4 * math.sin(psi)!r},{y0 + 0.4 * math.cos(psi)!r}", "--recover-dir",
           f"{math.cos(psi + math.pi / 18)!r},{math.sin(psi + math.pi / 18)!r}", "--recover-speed", "6"]
    recover = ["--bounds", *car, "--recover-len", "12.5"]
    fan = ["--bounds", *car, "--recover-fan", "2,12.5,40,2000"]
    alone["stop"] = _stage_run(src, tmp_path / "stop", stop)
    alone["retime"] = _stage_run(src, tmp_path / "retime", retime)
    alone["recover"] = _stage_run(src, tmp_path / "recover", recover)
    alone["fan"] = _stage_run(src, tmp_path / "fan", fan)
    # each stage alone said and wrote what it should: two lines, two files of its own
    own = {"rejoin": ("[rejoin]", "_from_v0"), "stop": ("[stop]", "_stop"), "retime": ("[retime]", "_retimed"),
           "recover": ("[recover]", "_recover"), "fan": ("[recover]", "_recover")}
    for name, (tag, suffix) in own.items():
        lines, files = alone[name]
        assert sum(ln.startswith(tag + " winner") for ln in lines) == 2, (name, lines)
        assert [f for f in files if f.endswith(suffix + ".csv")] == [f"t_centerline_trajectory_{q}{suffix}.csv" for q in range(2)]
        assert lines[-1].startswith("[best] ") and lines[-1] == alone["rejoin"][0][-1]
    assert sum(ln.startswith("[recover-fan] winner") for ln in alone["fan"][0]) == 2 * (4 + 1)
    assert not any(ln.startswith("[recover-fan]") for ln in alone["recover"][0])
    for tag, last, d in (("recover", recover, "all"), ("fan", fan, "all_fan")):
        lines, files = _stage_run(src, tmp_path / d, rejoin + stop + retime + last)
        parts = [alone["rejoin"], alone["stop"], alone["retime"], alone[tag]]
        # stderr: every stage's lines, verbatim, in stage order, then the one [best] line
        assert lines == [ln for ls, _ in parts for ln in ls[:-1]] + [alone["rejoin"][0][-1]], d
        # the files: exactly the union, each byte for byte what its stage alone wrote
        want = {}
        for _, fs in parts:
            for f, text in fs.items():
                assert want.setdefault(f, text) == text, f                 # (the shared files agree among the single runs)
        assert sorted(files) == sorted(want), d
        for f, text in want.items():
            assert files[f] == text, (d, f)
        assert len(files) == len(alone["rejoin"][1]) + 2 + 2 + 4 and len(alone["rejoin"][1]) >= 7
