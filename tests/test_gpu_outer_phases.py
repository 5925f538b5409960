"""The once-per-outer phases of the register-resident kernel (path update, normals, the exchange
into the corridor's chunk mapping, lin-geom and the output stores) against the CPU oracle, in
the throughput shapes: sizes around the chunk edges of the 64*CK-sample corridor chunks and of
the K-sample owner chunks, the iteration counts at which the only alpha_last store is the first
or the second update's, and the lap evaluation (per-instance centres, nothing iterates).
Tolerances and comparisons are test_gpu_parity's: 1e-4*max|ref| + 1e-9 per column, counters
exact, zeros with the oracle's sign."""
import numpy as np
import pytest

import oracle_lib as O
from practice_path_planning_for_formula_student_driverless_amd import abi, raceline
from test_gpu_parity import REL, _lib_or_skip, _synthetic, col_close, compare_outputs, zero_signs_equal

pytestmark = pytest.mark.gpu

MC, MT = abi.RL_MODE_MINCURV, abi.RL_MODE_MINTIME
SEEDS = np.array([0, 3], dtype=np.uint64)


def _run_thr(prob, cfgs, seeds, B, shape_B=1024):
    """One plan of both modes in the throughput shape a batch of shape_B instances gets."""
    pl = raceline.Plan(prob, cfgs, seeds=seeds, B=B, modes=MC | MT)
    try:
        pl.set_shape_batch(shape_B)
        shapes = (pl.shape(MC), pl.shape(MT))
        pl.run()
        return pl.fetch(), shapes
    finally:
        pl.close()


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("N", [8, 63, 65, 257, 511, 513, 1025, 2047, 2049, 4096])
def test_chunk_edges_vs_oracle(N, closed):
    """Ragged tails and chunk edges of the owner mapping (K samples per lane) and of the
    corridor's mapping (64*CK consecutive samples per wave), closed and open, seeds 0 and 3."""
    _lib_or_skip()
    prob = _synthetic(N, closed, np.random.default_rng(N))
    cfg = abi.default_cfg()
    cfg.max_outer_iters = 3
    cfg.max_inner_iters = 20
    (mc, mt), shapes = _run_thr(prob, cfg, SEEDS, len(SEEDS))
    assert all(K >= 4 for K, T in shapes), shapes            # a throughput shape, not a latency shape
    omc, omt = O.run_oracle(prob, cfg, seeds=SEEDS, B=len(SEEDS))
    compare_outputs(mc, omc, False, f"N{N}.mc")
    compare_outputs(mt, omt, True, f"N{N}.mt")


def test_cmap1_n2000_vs_reference_fixture():
    """The headline problem at seed 0 in the headline shape, against the reference's own outputs."""
    _lib_or_skip()
    case = O.load_case("cmap1_n2000")
    prob, cfg = O.case_problem(case), O.case_cfg(case)
    pl = raceline.Plan(prob, cfg, seeds=None, B=1, modes=MC)
    try:
        pl.set_shape_batch(1024)
        assert pl.shape(MC) == (8, 256)
        pl.run()
        mc, _ = pl.fetch()
    finally:
        pl.close()
    for f in abi.OUT_F64:
        col_close(getattr(mc, f)[0], case[f"mc_{f}"], f"cmap1_n2000.mc_{f}")
        zero_signs_equal(getattr(mc, f)[0], case[f"mc_{f}"], f"cmap1_n2000.mc_{f}")
    omc, _ = O.run_oracle(prob, cfg, B=1, modes=(True, False))
    np.testing.assert_array_equal(mc.evals, omc.evals)
    np.testing.assert_array_equal(mc.accepts, omc.accepts)


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("N", [261, 2000])
@pytest.mark.parametrize("max_outer", [0, 1, 2])
def test_alpha_columns_at_few_outer_iterations(max_outer, N, closed):
    """alpha_last is stored by the last update only and alpha_total starts from the first
    update's 0.0 + alpha: with one or two outer iterations those are the same or adjacent
    updates, with none both columns keep their zeros."""
    _lib_or_skip()
    prob = _synthetic(N, closed, np.random.default_rng(100 + N))
    cfg = abi.default_cfg()
    cfg.max_outer_iters = max_outer
    cfg.max_inner_iters = 20
    (mc, mt), _ = _run_thr(prob, cfg, SEEDS, len(SEEDS))
    omc, omt = O.run_oracle(prob, cfg, seeds=SEEDS, B=len(SEEDS))
    for got, ref, name in ((mc, omc, "mc"), (mt, omt, "mt")):
        for f in ("alpha_last", "alpha_total"):
            col_close(getattr(got, f), getattr(ref, f), f"mo{max_outer}.N{N}.{name}.{f}")
            zero_signs_equal(getattr(got, f), getattr(ref, f), f"mo{max_outer}.N{N}.{name}.{f}")
        if max_outer == 0:
            assert not np.any(got.alpha_last) and not np.any(got.alpha_total)
            assert not np.any(np.signbit(got.alpha_last)) and not np.any(np.signbit(got.alpha_total))
    compare_outputs(mc, omc, False, f"mo{max_outer}.N{N}.mc", counters=max_outer > 0)
    compare_outputs(mt, omt, True, f"mo{max_outer}.N{N}.mt", counters=max_outer > 0)


@pytest.mark.parametrize("closed", [True, False])
def test_lap_eval_per_instance_centres(closed):
    """Lap evaluation: every instance has its own centre line and length and nothing iterates
    (max_outer_iters = 0), so nothing of one instance may serve another."""
    _lib_or_skip()
    N = 513
    rng = np.random.default_rng(5)
    probs = [_synthetic(N, closed, rng) for _ in range(3)]
    paths = np.stack([p.center * (1.0 + 0.1 * i) for i, p in enumerate(probs)])
    Ls = [float(p.L) * (1.0 + 0.1 * i) for i, p in enumerate(probs)]
    cfg = abi.default_cfg()
    ev = raceline.lap_eval(paths, Ls, closed, cfg)
    for b in range(len(probs)):
        orc = O.run_oracle_lap_eval(paths[b], Ls[b], closed, cfg)
        assert abs(ev.lap[b] - orc.lap[0]) / orc.lap[0] <= REL
        for k in ("heading", "kappa", "v", "ax"):
            col_close(getattr(ev, k)[b], getattr(orc, k)[0], f"lap_eval.{b}.{k}")
            zero_signs_equal(getattr(ev, k)[b], getattr(orc, k)[0], f"lap_eval.{b}.{k}")
        np.testing.assert_array_equal(ev.vpass_sweeps[b], orc.vpass_sweeps[0][:1])
