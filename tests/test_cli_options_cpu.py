"""`fsd_raceline`'s option checks: every rejected invocation, its exit code and its whole stderr.

The centreline form checks its options before its first GPU call, so every case here ends without a
device: exit 1 with the usage text, exit 2 with the one `[ERR]` line of the first check that fails,
exit 3 for what the argument loop throws.  The expected (returncode, stderr) pairs are
tests/golden/cli_options/messages.json, recorded once (`python tests/test_cli_options_cpu.py
--record`) from the binary as it was before the checks moved into one function; the directory and
the program's path stand in it as {dir} and {exe}.  stderr is compared as a whole string, so the
order of the checks is pinned by the cases with two mistakes."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_host_cli as H  # noqa: E402

MESSAGES = os.path.join(H.GOLD, "cli_options", "messages.json")
# what the stage options need: a batch, its winners, the min-time rows and the ticks
S = ["--seeds", "16", "--best", "2", "--mode", "mintime", "--trajectory-dt", "0.05", "--trajectory-cap", "2048"]
SB = S + ["--bounds"]
FROM = ["--recover-from", "1,2"]
RT = ["--retime-set", "mu=0.8"]


def cases(N):
    """name -> arguments after `<exe> <centerline.csv>`; N: the samples of the closed centreline
    (an --open run keeps the closing row: N + 1 samples)."""
    L = ["--L", "100"]
    c = {
        # ---- exit 2: run_from_centerline's checks, in their order
        "inputs_no_L": [],                                          # no --L and no <base>_with_geom.csv
        "inputs_L_zero": ["--L", "0"],
        "inputs_L_negative": ["--L", "-5"],
        "score_unknown": L + ["--score", "fastest", "--seeds", "4", "--best", "2", "--mode", "mincurv"],
        "score_without_best": L + ["--score", "lap", "--seeds", "4", "--mode", "mincurv"],
        "score_without_seeds": L + ["--score", "default", "--best", "2", "--mode", "mincurv"],
        "score_lap_mintime": L + ["--score", "lap", "--seeds", "4", "--best", "2", "--mode", "mintime"],
        "score_lap_both": L + ["--score", "lap", "--seeds", "4", "--best", "2"],
        "traj_without_best": L + ["--seeds", "4", "--trajectory-dt", "0.05"],
        "traj_without_seeds": L + ["--best", "2", "--trajectory-dt", "0.05"],
        "traj_cap_alone": L + ["--trajectory-cap", "100"],
        "traj_dt_negative": L + S[:6] + ["--trajectory-dt", "-0.05"],
        "traj_dt_zero_with_cap": L + S[:6] + ["--trajectory-dt", "0", "--trajectory-cap", "100"],
        "traj_dt_inf": L + S[:6] + ["--trajectory-dt", "inf"],
        "traj_dt_nan": L + S[:6] + ["--trajectory-dt", "nan"],
        "traj_cap_negative": L + S[:8] + ["--trajectory-cap", "-1"],
        "traj_cap_above": L + S[:8] + ["--trajectory-cap", "1048577"],
        "start_without_traj": L + S[:6] + ["--start-speed", "0"],
        "start_mincurv": L + ["--seeds", "16", "--best", "2", "--mode", "mincurv", "--trajectory-dt", "0.05", "--start-speed", "0"],
        "start_negative": L + S + ["--start-speed", "-1"],
        "start_inf": L + S + ["--start-speed", "inf"],
        "stop_without_traj": L + S[:6] + ["--stop-sample", "10"],
        "stop_mincurv": L + ["--seeds", "16", "--best", "2", "--mode", "mincurv", "--trajectory-dt", "0.05", "--stop-sample", "10"],
        "stop_speed_alone": L + S + ["--stop-speed", "3"],
        "stop_from_alone": L + S + ["--stop-from", "60"],
        "stop_from_zero_alone": L + S + ["--stop-from", "0"],
        "stop_sample_minus_one": L + S + ["--stop-sample", "-1"],
        "stop_sample_minus_two": L + S + ["--stop-sample", "-2"],
        "stop_sample_N": L + S + ["--stop-sample", str(N)],
        "stop_sample_open_zero": L + S + ["--open", "--stop-sample", "0"],
        "stop_sample_open_above": L + S + ["--open", "--stop-sample", str(N + 1)],
        "stop_speed_negative": L + S + ["--stop-sample", "10", "--stop-speed", "-1"],
        "stop_speed_inf": L + S + ["--stop-sample", "10", "--stop-speed", "inf"],
        "stop_from_zero": L + S + ["--stop-sample", "10", "--stop-from", "0"],
        "stop_from_minus_one": L + S + ["--stop-sample", "10", "--stop-from", "-1"],
        "stop_from_negative": L + S + ["--stop-sample", "10", "--stop-from", "-5"],
        "retime_without_traj": L + S[:6] + RT,
        "retime_mincurv": L + ["--seeds", "16", "--best", "2", "--mode", "mincurv", "--trajectory-dt", "0.05"] + RT,
        "retime_from_alone": L + S + ["--retime-from", "3"],
        "retime_from_minus_one_alone": L + S + ["--retime-from", "-1"],
        "retime_from_minus_one": L + S + RT + ["--retime-from", "-1"],
        "retime_from_minus_two": L + S + RT + ["--retime-from", "-2"],
        "retime_from_N": L + S + RT + ["--retime-from", str(N)],
        "retime_from_open_last": L + S + RT + ["--open", "--retime-from", str(N)],
        "retime_unknown_knob": L + S + ["--retime-set", "no_such_knob=1"],
        "retime_second_knob_unknown": L + S + RT + ["--retime-set", "no_such_knob=1"],
        "recover_without_bounds": L + S + FROM,
        "recover_without_traj": L + S[:6] + ["--bounds"] + FROM,
        "recover_mincurv": L + ["--seeds", "16", "--best", "2", "--mode", "mincurv", "--trajectory-dt", "0.05", "--bounds"] + FROM,
        "recover_y_nan": L + SB + ["--recover-from", "1,nan"],
        "recover_x_inf": L + SB + ["--recover-from", "inf,2"],
        "recover_dir_nan": L + SB + FROM + ["--recover-dir", "nan,0"],
        "recover_dir_inf": L + SB + FROM + ["--recover-dir", "1,inf"],
        "recover_len_zero": L + SB + FROM + ["--recover-len", "0"],
        "recover_len_negative": L + SB + FROM + ["--recover-len", "-3"],
        "recover_len_nan": L + SB + FROM + ["--recover-len", "nan"],
        "recover_speed_nan": L + SB + FROM + ["--recover-speed", "nan"],
        "recover_speed_inf": L + SB + FROM + ["--recover-speed", "inf"],
        "fan_too_many": L + SB + FROM + ["--recover-fan", ",".join(["5"] * 17)],
        "fan_zero_length": L + SB + FROM + ["--recover-fan", "5,0"],
        "fan_nan_length": L + SB + FROM + ["--recover-fan", "5,nan"],
        "fan_without_from": L + SB + ["--recover-fan", "5,10"],
        "fan_second_replaces_first": L + SB + FROM + ["--recover-fan", "5,10", "--recover-fan", "5,-1"],
        "bounds_without_traj": L + S[:6] + ["--bounds"],
        "bounds_without_best": L + ["--seeds", "4", "--bounds"],
        "best_mode_both": L + ["--seeds", "4", "--best", "2"],
        "best_above_B": L + ["--seeds", "4", "--best", "5", "--mode", "mincurv"],
        "best_above_max": L + ["--seeds", "100", "--best", "65", "--mode", "mintime"],
        # ---- two mistakes: the earlier check reports
        "two_score_then_traj": L + ["--score", "fastest", "--trajectory-dt", "-1"],
        "two_traj_then_start": L + S[:6] + ["--trajectory-dt", "-1", "--start-speed", "-1"],
        "two_start_then_stop": L + S + ["--start-speed", "-1", "--stop-sample", str(N)],
        "two_stop_speed_then_from": L + S + ["--stop-sample", "10", "--stop-speed", "-1", "--stop-from", "0"],
        "two_stop_then_retime": L + S + ["--stop-from", "0", "--retime-from", "-1"],
        "two_retime_from_then_knob": L + S + ["--retime-set", "no_such_knob=1", "--retime-from", str(N)],
        "two_retime_then_recover": L + S + ["--retime-from", "3"] + FROM,
        "two_recover_then_fan": L + SB + ["--recover-from", "1,nan", "--recover-fan", "5,0"],
        "two_fan_then_bounds": L + S[:6] + ["--bounds", "--recover-fan", "5,10"],
        "two_bounds_then_best": L + ["--seeds", "4", "--best", "5", "--mode", "mincurv", "--bounds"],
        "two_best_mode_then_K": L + ["--seeds", "4", "--best", "5"],
        # a NaN reads as "not given" for the three options that a NaN once encoded
        "nan_start_is_absent": L + S + ["--start-speed", "nan", "--stop-speed", "-1"],
        "nan_stop_speed_is_absent": L + S + ["--stop-sample", "10", "--stop-speed", "nan", "--stop-from", "0"],
        "nan_L_is_absent": ["--L", "nan"],
        # ---- exit 3: what the argument loop throws
        "arg_missing_value": ["--L"],
        "arg_missing_value_last": L + ["--seeds", "4", "--recover-fan"],
        "arg_unknown_option": L + ["--no-such-option"],
        "arg_stod": ["--L", "abc"],
        "arg_stod_start_speed": L + ["--start-speed", "fast"],
        "arg_stoi": L + ["--seeds", "many"],
        "arg_stoi_out_of_range": L + ["--stop-sample", "99999999999"],
        "arg_stoi_devices": L + ["--devices", "0,x"],
        "arg_recover_from_no_comma": L + ["--recover-from", "12"],
        "arg_recover_dir_no_comma": L + ["--recover-dir", "12"],
        "arg_recover_from_stod": L + ["--recover-from", "1,y"],
        "arg_recover_fan_empty": L + ["--recover-fan", ""],
        "arg_recover_fan_stod": L + ["--recover-fan", "5,,6"],
        "arg_set_unknown_knob": L + ["--set", "no_such_knob=1"],
        "arg_first_mistake_wins": ["--L", "abc", "--no-such-option"],
    }
    return c


# exit 1: the positional count (no centreline argument in front of these)
USAGE = {"usage_bare": [], "usage_two_files": ["a.csv", "b.csv"], "usage_four_files": ["a.csv", "b.csv", "c.csv", "d.csv"],
         "usage_options_only": ["--seeds", "4"]}


@pytest.fixture(scope="module")
def centreline(tmp_path_factory):
    """Steps 1-5 on training_map, once: the three files the centreline form reads."""
    d = tmp_path_factory.mktemp("cli_options")
    r, _ = H._run("training_map", d, ["--stop-after", "centerline"])
    assert r.returncode == 0, r.stderr
    with open(d / "t_centerline.csv") as f:
        rows = len([ln for ln in f.read().splitlines() if ln])
    return d, rows - 1                                             # (the closing row repeats the first)


def _invocations(d, N):
    cen = str(d / "t_centerline.csv")
    inv = {name: [cen, *a] for name, a in cases(N).items()}
    inv.update(USAGE)
    inv["inputs_no_such_centreline"] = [str(d / "absent.csv"), "--L", "100"]
    return inv


def _run(d, argv):
    r = subprocess.run([H._exe(), *argv], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    return r.returncode, r.stderr.replace(H._exe(), "{exe}").replace(str(d), "{dir}"), r.stdout


def test_every_rejected_invocation_reports_as_recorded(centreline):
    d, N = centreline
    with open(MESSAGES) as f:
        want = json.load(f)
    assert want["N"] == N
    inv = _invocations(d, N)
    assert sorted(inv) == sorted(want["cases"])
    before = sorted(os.listdir(d))
    got = {}
    for name, argv in inv.items():
        rc, err, out = _run(d, argv)
        got[name] = {"rc": rc, "stderr": err}
        assert out == "", name
    for name in inv:
        assert got[name] == want["cases"][name], name
    assert sorted(os.listdir(d)) == before                         # a rejected invocation writes nothing
    # the recording covers what it should: each exit code, and a single [ERR] line for 2 and 3
    codes = [v["rc"] for v in want["cases"].values()]
    assert set(codes) == {1, 2, 3} and codes.count(2) >= 70 and codes.count(3) >= 12
    for name, v in want["cases"].items():
        assert ": no HIP device" not in v["stderr"] and "rl_" not in v["stderr"], name    # none reached the library
        if name.startswith("usage_"):
            assert v["rc"] == 1 and v["stderr"].startswith("Usage: {exe} inner.csv outer.csv centerline.csv"), name
        elif name.startswith("arg_"):
            assert v["rc"] == 3 and v["stderr"].startswith("[ERR] ") and v["stderr"].count("\n") == 1, name
        elif name != "inputs_no_such_centreline":
            assert v["rc"] == 2 and v["stderr"].startswith("[ERR] ") and v["stderr"].count("\n") == 1, name


def test_the_sentinel_inputs_land_on_their_messages(centreline):
    """-1, 0 and -1 once stood for "not given" inside the program; given on the command line they
    are values like any other."""
    d, N = centreline
    cen = str(d / "t_centerline.csv")
    for extra, text in ((["--stop-sample", "-1"], f"[ERR] --stop-sample J: a sample of the raceline, 0..{N - 1}\n"),
                        (["--stop-sample", "10", "--stop-from", "0"], "[ERR] --stop-from K: >= 1\n"),
                        (RT + ["--retime-from", "-1"],
                         f"[ERR] --retime-from S: a sample of the raceline with one ahead, 0..{N - 1}\n")):
        rc, err, _ = _run(d, [cen, "--L", "100", *S, *extra])
        assert (rc, err) == (2, text), extra


if __name__ == "__main__" and "--record" in sys.argv:
    import pathlib
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        d = pathlib.Path(tmp)
        r, _ = H._run("training_map", d, ["--stop-after", "centerline"])
        assert r.returncode == 0, r.stderr
        with open(d / "t_centerline.csv") as f:
            N = len([ln for ln in f.read().splitlines() if ln]) - 1
        rec = {}
        for name, argv in _invocations(d, N).items():
            rc, err, _ = _run(d, argv)
            rec[name] = {"rc": rc, "stderr": err}
    os.makedirs(os.path.dirname(MESSAGES), exist_ok=True)
    with open(MESSAGES, "w") as f:
        json.dump({"N": N, "cases": rec}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} cases, N = {N}")
