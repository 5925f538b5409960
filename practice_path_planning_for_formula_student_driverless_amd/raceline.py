"""Host-side mirror of the reference's raceline interface, over the C-ABI.

Reference (``ref`` = /root/reference/src/main.cpp):

* :func:`compute_min_curvature_raceline` — ``raceline_min_curv::compute_min_curvature_raceline``
  (ref:683-764): same arguments (center, innerE, outerE, veh_width, L, closed),
  same :class:`MinCurvResult` fields (raceline, heading, curvature,
  alpha_total, alpha_last; ref:677-681).
* :func:`compute_min_time_raceline` — ``raceline_min_time::compute_min_time_raceline``
  (ref:905-1052), :class:`MinTimeResult` adds v, ax, lap_time (ref:897-903).
* :func:`ring_edges` / :func:`polyline_edges` — ``edges::ringEdges`` / ``polylineEdges`` (ref:251-260).
* :func:`compute_raceline_and_save` / :func:`compute_mintime_and_save` — the
  pipeline callers and their CSV writers (ref:1337-1438), same file names,
  headers and ``precision(9)`` fixed formatting.
* ``cfg`` — :func:`default_cfg` holds ``cfg::Config``'s hot-path knobs (ref:77-113).

Beyond the reference: :func:`optimize_batch` and :class:`Plan` run B
instances (α-seeds, cfg sweeps) in one launch; that is the product.
:func:`optimize_best` / :meth:`Plan.select` rank the batch on the GPU and
return only the k best instances of each group.
:func:`best_trajectory` / :meth:`Plan.trajectory` resample racelines on the GPU into what a
controller tracks, the state at every control tick; :func:`trajectory_host` is their
specification in NumPy.
:func:`horizon` / :meth:`Plan.horizon` locate poses on those trajectories' rows and resample
the next ticks from there, across the start line on a closed track; :func:`horizon_host` is
their specification in NumPy.
:func:`bounds` / :meth:`Plan.bounds` cast the free track width about every sample of those rows,
and :meth:`Plan.horizon_bounds` takes it to the horizon's ticks; :func:`normals_host` and
:func:`horizon_bounds_host` state the two new pieces in NumPy.

Every compute call goes through ``librl.so`` (HIP, gfx950).  With no GPU the
calls raise :class:`RacelineError` (RL_ENODEV): there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import abi
from .abi import GeomProblem, Outputs, Problem, RlCfg, default_cfg, set_mu  # noqa: F401


class RacelineError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rl error {code}: {msg}")
        self.code = code


def _lib():
    return abi.load_library()


def _check(rc: int) -> None:
    if rc != 0:
        raise RacelineError(rc, _lib().rl_last_error().decode(errors="replace"))


# ------------------------------------------------------------------ geometry
def ring_edges(ring: np.ndarray) -> np.ndarray:
    """edges::ringEdges (ref:251-255): n segments, the last one closing the ring."""
    ring = np.ascontiguousarray(ring, dtype=np.float64).reshape(-1, 2)
    n = len(ring)
    if n == 0:
        return np.zeros((0, 4))
    return np.concatenate([ring, np.roll(ring, -1, axis=0)], axis=1)


def polyline_edges(ring: np.ndarray) -> np.ndarray:
    """edges::polylineEdges (ref:256-260): n-1 segments."""
    ring = np.ascontiguousarray(ring, dtype=np.float64).reshape(-1, 2)
    if len(ring) < 2:
        return np.zeros((0, 4))
    return np.concatenate([ring[:-1], ring[1:]], axis=1)


def edges_for(ring: np.ndarray, closed: bool) -> np.ndarray:
    return ring_edges(ring) if closed else polyline_edges(ring)


# ------------------------------------------------------------------ results
@dataclass
class MinCurvResult:
    """raceline_min_curv::Result (ref:677-681)."""

    raceline: np.ndarray      # [N,2]
    heading: np.ndarray
    curvature: np.ndarray
    alpha_total: np.ndarray
    alpha_last: np.ndarray
    evals: Optional[np.ndarray] = None


@dataclass
class MinTimeResult(MinCurvResult):
    """raceline_min_time::Result (ref:897-903)."""

    v: Optional[np.ndarray] = None
    ax: Optional[np.ndarray] = None
    lap_time: float = 0.0
    vpass_sweeps: Optional[np.ndarray] = None


# ------------------------------------------------------------------ batch API
def _check_batch(B: int, ncfg: int, seeds) -> None:
    """The C side reads exactly B seeds and B (or 1) cfgs (rl_abi.h): a shorter array
    would be read past its end, so a mismatch is an error here."""
    if B < 0:
        raise ValueError(f"B must be >= 0, got {B}")
    if ncfg not in (1, B):
        raise ValueError(f"cfgs: need 1 or B={B} entries, got {ncfg}")
    if seeds is not None and len(seeds) != B:
        raise ValueError(f"seeds: need exactly B={B} entries, got {len(seeds)}")


def optimize_batch(prob: Problem, cfgs, seeds=None, B: Optional[int] = None,
                   mincurv: bool = True, mintime: bool = True, devices: Optional[Sequence[int]] = None,
                   out=None):
    """Optimise B instances (seed b / cfg b) of one problem on the GPU.

    cfgs: one RlCfg (broadcast) or a list of B.  seeds: None (all zero — the
    reference exactly) or B uint64 seeds.  devices: None (the current device) or a
    list of device indices: contiguous instance blocks, one per device
    (rl_optimize_multi).  out: None (fresh output arrays from abi.HOST_POOL, which
    recycles the buffers of earlier results the caller has dropped) or the
    (Outputs|None, Outputs|None) of an earlier call of the same shape, written in place
    (a caller that keeps its buffers, as the C ABI's callers own theirs).  Returns
    (Outputs|None, Outputs|None).
    """
    cfg_arr, ncfg = abi.cfg_array(cfgs)
    if B is None:
        B = ncfg if ncfg > 1 else (len(seeds) if seeds is not None else 1)
    _check_batch(B, ncfg, seeds)
    mo = int(cfg_arr[0].max_outer_iters)
    seeds_a = abi.seed_array(seeds)
    if out is not None:
        out_mc, out_mt = out
        for o, want, mt in ((out_mc, mincurv, False), (out_mt, mintime, True)):
            if (o is not None) != want:
                raise ValueError("out: one Outputs per requested mode (None for the others)")
            if o is not None and (o.x.shape != (B, prob.N) or o.evals.shape != (B, mo) or (mt and o.lap is None)
                                  or not all(getattr(o, f).flags.c_contiguous for f in abi.OUT_F64)):
                raise ValueError("out: Outputs of a different shape or mode")
    else:
        # every element is written by the call (no zeroing of memory about to be overwritten);
        # buffers recycled from arrays of earlier calls that the caller has dropped
        out_mc = Outputs.alloc(B, prob.N, mo, False, zero=False, pool=abi.HOST_POOL) if mincurv else None
        out_mt = Outputs.alloc(B, prob.N, mo, True, zero=False, pool=abi.HOST_POOL) if mintime else None
    c_mc = out_mc.as_c() if out_mc else None
    c_mt = out_mt.as_c() if out_mt else None
    p = prob.as_c()
    if devices is None:
        _check(_lib().rl_optimize(C.byref(p), cfg_arr, ncfg, abi.u64ptr(seeds_a), B,
                                  C.byref(c_mc) if c_mc else None, C.byref(c_mt) if c_mt else None))
    else:
        devs = np.ascontiguousarray(np.asarray(list(devices), dtype=np.int32))
        _check(_lib().rl_optimize_multi(C.byref(p), cfg_arr, ncfg, abi.u64ptr(seeds_a), B,
                                        devs.ctypes.data_as(C.POINTER(C.c_int32)), len(devs),
                                        C.byref(c_mc) if c_mc else None, C.byref(c_mt) if c_mt else None))
    return out_mc, out_mt


# ------------------------------------------------------ best k of a batch
@dataclass
class Selected:
    """The k best instances of each of G groups (rl_plan_select / rl_optimize_best):
    index [G, k] global instance indices, best first; score [G, k] their scores; scores [B]
    every instance's score (min-time: the lap; min-curvature: h * sum kappa^2, or the lap
    stage's lap with score="lap"); out: Outputs
    with G*k rows, row g*k + r = instance index[g, r]."""

    index: np.ndarray
    score: np.ndarray
    scores: np.ndarray
    out: Outputs


_MODES = {"mincurv": abi.RL_MODE_MINCURV, "mintime": abi.RL_MODE_MINTIME,
          abi.RL_MODE_MINCURV: abi.RL_MODE_MINCURV, abi.RL_MODE_MINTIME: abi.RL_MODE_MINTIME}


def _check_select(B: int, mode, k: int, group_size) -> tuple:
    """(mode bit, group size) of a selection over B instances; the C side writes G*k entries
    into arrays sized from these numbers, so a mismatch is an error here."""
    if mode not in _MODES:
        raise ValueError(f"mode must be 'mincurv' or 'mintime', got {mode!r}")
    if B < 1:
        raise ValueError(f"B must be >= 1, got {B}")
    gs = B if group_size in (None, 0) else int(group_size)
    if gs < 1 or gs > B or B % gs != 0:
        raise ValueError(f"group_size: B={B} is not a multiple of {gs}")
    if not 1 <= k <= min(gs, abi.RL_SELECT_MAX_K):
        raise ValueError(f"k: need 1 <= k <= min(group_size={gs}, {abi.RL_SELECT_MAX_K}), got {k}")
    return _MODES[mode], gs


_SCORES = {"default": abi.RL_SCORE_DEFAULT, "lap": abi.RL_SCORE_LAP,
           abi.RL_SCORE_DEFAULT: abi.RL_SCORE_DEFAULT, abi.RL_SCORE_LAP: abi.RL_SCORE_LAP}


def _check_score(score, mode_bit: int) -> bool:
    """True if the selection ranks the lap stage's lap (score 'lap' on min-curvature results)."""
    if score not in _SCORES:
        raise ValueError(f"score must be 'default' or 'lap', got {score!r}")
    return _SCORES[score] == abi.RL_SCORE_LAP and mode_bit == abi.RL_MODE_MINCURV


def _selected_alloc(B: int, N: int, mo: int, mode: int, k: int, gs: int, lap: bool = False) -> Selected:
    G = B // gs
    out = Outputs.alloc(G * k, N, mo, mode == abi.RL_MODE_MINTIME)
    if lap:                     # a min-curvature selection by lap: the lap stage's v, ax, lap, sweeps [G*k, 1]
        out.v, out.ax = np.zeros((G * k, N)), np.zeros((G * k, N))
        out.lap, out.vpass_sweeps = np.zeros(G * k), np.zeros((G * k, 1), dtype=np.int32)
    return Selected(index=np.zeros((G, k), dtype=np.int32), score=np.zeros((G, k)), scores=np.zeros(B), out=out)


def optimize_best(prob: Problem, cfgs, seeds=None, B: Optional[int] = None, mode="mintime", k: int = 1,
                  group_size: Optional[int] = None, score="default") -> Selected:
    """Optimise B instances in `mode` and return only the k best of each group of
    group_size (None: one group) instances, ranked and compacted on the GPU
    (rl_optimize_best): G*k rows are downloaded instead of B.  score: "default" (the lap
    for min-time, h * sum kappa^2 for min-curvature) or "lap": min-curvature racelines are
    ranked by the lap time of the lap stage (rl_optimize_best_scored), whose v, ax, lap and
    vpass_sweeps [G*k, 1] then come back with the winners' rows."""
    cfg_arr, ncfg = abi.cfg_array(cfgs)
    if B is None:
        B = ncfg if ncfg > 1 else (len(seeds) if seeds is not None else 1)
    _check_batch(B, ncfg, seeds)
    m, gs = _check_select(B, mode, k, group_size)
    if prob.N == 0:
        raise ValueError("optimize_best: N == 0 (nothing to rank)")
    by_lap = _check_score(score, m)
    sel = _selected_alloc(B, prob.N, int(cfg_arr[0].max_outer_iters), m, k, gs, by_lap)
    seeds_a = abi.seed_array(seeds)
    p = prob.as_c()
    o = sel.out.as_c()
    s = abi.RlSelect(m, k, gs, 0)
    if _SCORES[score] == abi.RL_SCORE_DEFAULT:
        _check(_lib().rl_optimize_best(C.byref(p), cfg_arr, ncfg, abi.u64ptr(seeds_a), B, C.byref(s),
                                       abi.iptr(sel.index), abi.dptr(sel.score), abi.dptr(sel.scores), C.byref(o)))
    else:
        _check(_lib().rl_optimize_best_scored(C.byref(p), cfg_arr, ncfg, abi.u64ptr(seeds_a), B, C.byref(s),
                                              _SCORES[score], abi.iptr(sel.index), abi.dptr(sel.score),
                                              abi.dptr(sel.scores), C.byref(o)))
    return sel


# ------------------------------------------------- trajectories: racelines by time
TRAJ_HEADER = "t,s,x,y,heading_rad,curvature,v_mps,ax_mps2\n"


@dataclass
class Trajectory:
    """Time-stamped trajectories of R rows (rl_traj): the state at the ticks tau_m = m * dt.
    s, x, y, heading, kappa, v, ax [R, M_cap]; stamps [R, N + 1] (t_i: when the car is at
    sample i); T [R] (closed rows: the lap, summed serially); count [R]: row r holds count[r]
    ticks, the entries after them are unspecified."""

    s: np.ndarray
    x: np.ndarray
    y: np.ndarray
    heading: np.ndarray
    kappa: np.ndarray
    v: np.ndarray
    ax: np.ndarray
    stamps: np.ndarray
    T: np.ndarray
    count: np.ndarray
    dt: float

    _C, _NODES = abi.RlTraj, ()          # (Plan._stage_fetch)

    @classmethod
    def alloc(cls, R: int, N: int, m_cap: int, dt: float) -> "Trajectory":
        cols = {n: np.zeros((R, m_cap)) for n in abi.TRAJ_COLS}
        return cls(**cols, stamps=np.zeros((R, N + 1)), T=np.zeros(R), count=np.zeros(R, dtype=np.int32), dt=float(dt))

    def as_c(self) -> abi.RlTraj:
        t = abi.RlTraj()
        for n in abi.TRAJ_COLS + ("stamps", "T"):
            setattr(t, n, _ptr(getattr(self, n), np.float64, n))
        t.count = _ptr(self.count, np.int32, "count")
        return t

    def row(self, r: int) -> dict:
        """The ticks of row r: t [count[r]] = m * dt and the seven columns' first count[r] entries."""
        m = int(self.count[r])
        out = {"t": np.arange(m, dtype=np.float64) * self.dt}
        for n in abi.TRAJ_COLS:
            out[n] = getattr(self, n)[r, :m]
        return out

    def table(self, r: int) -> np.ndarray:
        """[count[r], 8]: the rows of <base>_trajectory_<r>.csv (TRAJ_HEADER's columns)."""
        t = self.row(r)
        return np.stack([t[n] for n in ("t",) + abi.TRAJ_COLS], axis=1)


def _ptr(a: np.ndarray, dtype, name: str):
    """C pointer to a; the library reads and writes whole arrays through it, so anything but a
    C-contiguous array of `dtype` is an error here."""
    if not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags.c_contiguous:
        raise ValueError(f"{name}: need a C-contiguous {np.dtype(dtype).name} array")
    return a.ctypes.data_as(C.POINTER(C.c_int32 if dtype == np.int32 else C.c_double))


def _traj_rows(x, y, heading, kappa, v, ax, h) -> tuple:
    """The six rows as [B, N] float64 arrays of one shape and h as [B]."""
    rows = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, heading, kappa, v, ax)]
    if rows[0].ndim == 1:
        rows = [a[None] if a.ndim == 1 else a for a in rows]
    shape = rows[0].shape
    if len(shape) != 2 or shape[0] < 1 or any(a.shape != shape for a in rows):
        raise ValueError(f"trajectory: x, y, heading, kappa, v, ax must be [B, N] arrays of one shape, got "
                         f"{[a.shape for a in rows]}")
    hs = np.asarray(h, dtype=np.float64)
    if hs.ndim > 1 or (hs.ndim == 1 and hs.shape[0] != shape[0]):
        raise ValueError(f"trajectory: h must be a number or [B={shape[0]}] array, got shape {hs.shape}")
    return rows, np.ascontiguousarray(np.broadcast_to(hs, (shape[0],)))


def _check_ticks(dt, m_cap) -> None:
    if not (np.isfinite(dt) and dt > 0):
        raise ValueError(f"dt must be finite and > 0, got {dt}")
    if not 1 <= int(m_cap) <= abi.RL_TRAJ_MAX_TICKS:
        raise ValueError(f"m_cap must be 1..{abi.RL_TRAJ_MAX_TICKS}, got {m_cap}")


def trajectory_host(x, y, heading, kappa, v, ax, h, closed: bool, dt: float, m_cap: int) -> Trajectory:
    """The specification of the trajectory stage (include/rl_abi.h) in NumPy; the
    kernel equals it bit for bit.  Rows [B, N] (or one row [N]), h a number or [B].  Per row:
    stamps t = cumsum([0, h / smax(1e-6, v_i) ...]) (np.cumsum adds serially in index order),
    T = t[S] with S = N segments (closed) or N - 1 (open); ticks tau_m = m * dt, M = min(m_cap,
    #{tau_m < T}) (0 for a NaN or infinite T); segment i = searchsorted(t, tau, "right") - 1,
    u = (tau - t_i) / (t_{i+1} - t_i); the columns interpolate between samples i and
    j = (i + 1) mod N, the heading along the shorter arc, ax constant on the segment."""
    rows, hs = _traj_rows(x, y, heading, kappa, v, ax, h)
    _check_ticks(dt, m_cap)
    B, N = rows[0].shape
    m_cap, closed, dt = int(m_cap), bool(closed), float(dt)
    out = Trajectory.alloc(B, N, m_cap, dt)
    tau_all = np.arange(m_cap, dtype=np.float64) * dt
    S = N if closed else N - 1
    for b in range(B):
        X, Y, P, K, V, A = (a[b] for a in rows)
        hb = hs[b]
        with np.errstate(all="ignore"):
            inc = hb / np.where(1e-6 < V, V, 1e-6)                 # smax(1e-6, v): (1e-6 < v) ? v : 1e-6
            t = np.cumsum(np.concatenate(([0.0], inc)))            # t_0 = 0, t_{i+1} = t_i + inc_i
            out.stamps[b] = t
            T = t[S] if N > 0 else 0.0
            out.T[b] = T
            M = int(np.count_nonzero(tau_all < T)) if np.isfinite(T) else 0
            out.count[b] = M
            if M == 0:
                continue
            tau = tau_all[:M]
            i = np.clip(np.searchsorted(t[:S + 1], tau, side="right") - 1, 0, S - 1)
            j = (i + 1) % N
            u = (tau - t[i]) / (t[i + 1] - t[i])
            d = P[j] - P[i]
            d = np.where(d > np.pi, d - 2.0 * np.pi, np.where(d < -np.pi, d + 2.0 * np.pi, d))
            out.s[b, :M] = (i.astype(np.float64) + u) * hb
            out.x[b, :M] = X[i] + u * (X[j] - X[i])
            out.y[b, :M] = Y[i] + u * (Y[j] - Y[i])
            out.heading[b, :M] = P[i] + u * d
            out.kappa[b, :M] = K[i] + u * (K[j] - K[i])
            out.v[b, :M] = V[i] + u * (V[j] - V[i])
            out.ax[b, :M] = A[i]
    return out


def trajectory(x, y, heading, kappa, v, ax, h, closed: bool, dt: float, m_cap: int, device: int = 0) -> Trajectory:
    """trajectory_host on the GPU (rl_trajectory): the trajectories of B given rows [B, N] (or
    one row [N]) with steps h (a number or [B]), row r of the result from row r."""
    rows, hs = _traj_rows(x, y, heading, kappa, v, ax, h)
    _check_ticks(dt, m_cap)
    B, N = rows[0].shape
    out = Trajectory.alloc(B, N, int(m_cap), dt)
    if N == 0:                              # (no row to point at)
        rows = [np.zeros((B, 1))] * 6
    t = out.as_c()
    _check(_lib().rl_trajectory(*[_ptr(a, np.float64, "row") for a in rows], _ptr(hs, np.float64, "h"), N, B,
                                1 if closed else 0, float(dt), int(m_cap), int(device), C.byref(t)))
    return out


_TRAJ_ROWS = {"all": abi.RL_TRAJ_ALL, "selected": abi.RL_TRAJ_SELECTED}


def best_trajectory(prob: Problem, cfgs, seeds=None, B: Optional[int] = None, mode="mintime", k: int = 1,
                    group_size: Optional[int] = None, score="default", dt: float = 0.05, m_cap: int = 1024):
    """optimize_best, then the winners' trajectories at ticks of dt seconds, at most m_cap per
    winner, resampled on the GPU and downloaded with the winners' rows in one pass
    (rl_optimize_best_trajectory).  Returns (Selected, Trajectory): row g*k + r of both is
    instance index[g, r].  A min-curvature trajectory takes v, ax, heading and curvature from
    the lap stage, whatever the score."""
    cfg_arr, ncfg = abi.cfg_array(cfgs)
    if B is None:
        B = ncfg if ncfg > 1 else (len(seeds) if seeds is not None else 1)
    _check_batch(B, ncfg, seeds)
    m, gs = _check_select(B, mode, k, group_size)
    if prob.N == 0:
        raise ValueError("best_trajectory: N == 0 (nothing to rank)")
    by_lap = _check_score(score, m)
    _check_ticks(dt, m_cap)
    sel = _selected_alloc(B, prob.N, int(cfg_arr[0].max_outer_iters), m, k, gs, by_lap)
    traj = Trajectory.alloc((B // gs) * k, prob.N, int(m_cap), dt)
    seeds_a = abi.seed_array(seeds)
    p = prob.as_c()
    o = sel.out.as_c()
    t = traj.as_c()
    s = abi.RlSelect(m, k, gs, 0)
    _check(_lib().rl_optimize_best_trajectory(C.byref(p), cfg_arr, ncfg, abi.u64ptr(seeds_a), B, C.byref(s),
                                              _SCORES[score], abi.iptr(sel.index), abi.dptr(sel.score),
                                              abi.dptr(sel.scores), C.byref(o), float(dt), int(m_cap), C.byref(t)))
    return sel, traj


# ------------------------------------------------- horizons: look-ahead from the car's pose
@dataclass
class Horizon:
    """The horizons of Q query poses (rl_hzn).  Location [Q]: seg (the segment the pose lies
    nearest to, -1: none), u (the foot's parameter on it), dist2 (squared distance), e (lateral
    offset, left of travel positive), t0 and s0 (the foot's time and arc length on the row);
    count [Q] ticks at t0 + m * dt in s, x, y, heading, kappa, v, ax [Q, M_cap], the entries
    after them unspecified.  On a closed row the ticks run on across the start line and s keeps
    growing."""

    s: np.ndarray
    x: np.ndarray
    y: np.ndarray
    heading: np.ndarray
    kappa: np.ndarray
    v: np.ndarray
    ax: np.ndarray
    u: np.ndarray
    t0: np.ndarray
    s0: np.ndarray
    e: np.ndarray
    dist2: np.ndarray
    seg: np.ndarray
    count: np.ndarray
    dt: float

    # What a pose-query result class holds, by shape: _C its ctypes struct, whose fields are _COLS
    # float64 [Q, m_cap], _PER float64 [Q], _INTS int32 [Q], _NODES float64 [Q, k_cap + 1] and the
    # candidates' _TAB_PER float64 and _TAB_INTS int32 [Q, n_cand]; _HOST_INTS and _HOST_NODES are
    # filled on the host side only.  Subclasses declare the tuples and inherit alloc and as_c.
    _C = abi.RlHzn
    _COLS = abi.TRAJ_COLS
    _PER = abi.HZN_LOC
    _INTS = ("seg", "count")
    _NODES = _TAB_PER = _TAB_INTS = _HOST_INTS = _HOST_NODES = ()

    @classmethod
    def alloc(cls, Q: int, m_cap: int, dt: float, k_cap: int = 1, n_cand: int = 1):
        groups = ((cls._COLS, (Q, m_cap), np.float64), (cls._PER, (Q,), np.float64), (cls._INTS + cls._HOST_INTS, (Q,), np.int32),
                  (cls._NODES + cls._HOST_NODES, (Q, k_cap + 1), np.float64), (cls._TAB_INTS, (Q, n_cand), np.int32),
                  (cls._TAB_PER, (Q, n_cand), np.float64))
        return cls(**{n: np.zeros(shape, dtype=t) for names, shape, t in groups for n in names}, dt=float(dt))

    def as_c(self):
        t = self._C()
        for n in self._COLS + self._PER + self._NODES + self._TAB_PER:
            setattr(t, n, _ptr(getattr(self, n), np.float64, n))
        for n in self._INTS + self._TAB_INTS:
            setattr(t, n, _ptr(getattr(self, n), np.int32, n))
        return t

    def row(self, q: int) -> dict:
        """The ticks of query q: t [count[q]] = t0[q] + m * dt and the seven columns' first count[q] entries."""
        m = int(self.count[q])
        out = {"t": self.t0[q] + np.arange(m, dtype=np.float64) * self.dt}
        for n in abi.TRAJ_COLS:
            out[n] = getattr(self, n)[q, :m]
        return out

    def table(self, q: int) -> np.ndarray:
        """[count[q], 8]: TRAJ_HEADER's columns for query q."""
        t = self.row(q)
        return np.stack([t[n] for n in ("t",) + abi.TRAJ_COLS], axis=1)


def _hzn_query(poses, row, seg_hint, window, dt, m_cap) -> tuple:
    """The query as arrays: poses [Q, 2] float64, row and seg_hint [Q] int32 or None."""
    P = np.ascontiguousarray(poses, dtype=np.float64)
    if P.ndim == 1 and P.shape[0] == 2:
        P = P[None]
    if P.ndim != 2 or P.shape[1] != 2 or not 1 <= P.shape[0] <= abi.RL_HZN_MAX_QUERIES:
        raise ValueError(f"horizon: poses must be [Q, 2] with 1 <= Q <= {abi.RL_HZN_MAX_QUERIES}, got shape {P.shape}")
    Q = P.shape[0]

    def ints(a, name):
        if a is None:
            return None
        a = np.asarray(a)
        if a.ndim == 0:
            a = np.broadcast_to(a, (Q,))
        if a.shape != (Q,) or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"horizon: {name} must be an integer or [Q={Q}] integers, got {a.dtype} {a.shape}")
        return np.ascontiguousarray(a, dtype=np.int32)

    if int(window) != window or window < 0 or window >= 2 ** 31:
        raise ValueError(f"horizon: window must be an integer >= 0, got {window}")
    _check_ticks(dt, m_cap)
    return P, ints(row, "row"), ints(seg_hint, "seg_hint")


def _hzn_c(P, rw, hint, window, dt, m_cap) -> abi.RlHznQuery:
    return abi.RlHznQuery(_ptr(P, np.float64, "poses"), None if rw is None else _ptr(rw, np.int32, "row"),
                          None if hint is None else _ptr(hint, np.int32, "seg_hint"), P.shape[0], int(window),
                          int(m_cap), 0, float(dt))


def _hzn_stamps(rows, hs, stamps):
    """The stamps [B, N + 1] of the rows: trajectory_host's, unless given (a plan's, as fetched)."""
    B, N = rows[0].shape
    if stamps is None:
        with np.errstate(all="ignore"):
            inc = hs[:, None] / np.where(1e-6 < rows[4], rows[4], 1e-6)
            return np.cumsum(np.concatenate((np.zeros((B, 1)), inc), axis=1), axis=1)
    stamps = np.ascontiguousarray(stamps, dtype=np.float64).reshape(-1, N + 1)
    if stamps.shape[0] != B:
        raise ValueError(f"horizon: stamps must be [B={B}, N + 1], got {stamps.shape}")
    return stamps


def _open_query(what: str, rows7, query) -> tuple:
    """What the pose-query stages' specifications and one-shot entries open with: the rows and
    steps (_traj_rows), the query as query() builds it, and B and N >= 1."""
    rows, hs = _traj_rows(*rows7)
    qy = query()
    B, N = rows[0].shape
    if N < 1:
        raise ValueError(f"{what}: N == 0 (no row)")
    return rows, hs, qy, B, N


def _query_rows(what: str, rows7, closed: bool, query, stamps, check=None) -> tuple:
    """The prologue of horizon_host, rejoin_host and stop_host: _open_query, row and seg_hint
    with their defaults and in range, the stage's own check(N, query) if any, and the stamps.
    Returns rows, hs, stamps [B, N + 1], N, S and the query with row and seg_hint filled in."""
    rows, hs, qy, B, N = _open_query(what, rows7, query)
    P, rw, hint = qy[:3]
    Q, S = P.shape[0], N if closed else N - 1
    rw = np.zeros(Q, dtype=np.int32) if rw is None else rw
    hint = np.full(Q, -1, dtype=np.int32) if hint is None else hint
    if np.any(rw < 0) or np.any(rw >= B):
        raise ValueError(f"{what}: row outside [0, {B})")
    if np.any(hint < -1) or np.any(hint >= S):
        raise ValueError(f"{what}: seg_hint outside [-1, {S})")
    if check is not None:
        check(N, qy)
    return rows, hs, _hzn_stamps(rows, hs, stamps), N, S, (P, rw, hint) + tuple(qy[3:])


def _one_shot(symbol: str, rows, hs, N: int, B: int, closed: bool, qc, out, device: int):
    """The one-shot C entry `symbol` (rl_horizon, rl_rejoin, rl_stop) on the B given rows with
    the query struct qc, into out."""
    oc = out.as_c()
    _check(getattr(_lib(), symbol)(*[_ptr(a, np.float64, "row") for a in rows], _ptr(hs, np.float64, "h"), N, B,
                                   1 if closed else 0, C.byref(qc), int(device), C.byref(oc)))
    return out


def _hzn_locate(X, Y, t, hb, px, py, g: int, W: int, closed: bool):
    """The horizon stage's candidates, distance, winner and location of one pose on one row:
    (seg, u, dist2, e, t0, s0), or None for a NaN winner or no candidate at all (a hint past an
    open row, which only the rollout stage's query admits)."""
    N = X.shape[0]
    S = N if closed else N - 1
    if g < 0 or (closed and 2 * W + 1 >= S):
        cand = np.arange(S)
    elif closed:
        cand = (g + np.arange(-W, W + 1)) % S
    else:
        cand = np.arange(max(0, g - W), min(S - 1, g + W) + 1)
    if cand.shape[0] == 0:
        return None
    with np.errstate(all="ignore"):
        i = cand
        j = (i + 1) % N
        dx, dy, wx, wy = X[j] - X[i], Y[j] - Y[i], px - X[i], py - Y[i]
        dd = dx * dx + dy * dy
        c = wx * dx + wy * dy
        ratio = c / dd
        lo = np.where(0.0 < ratio, ratio, 0.0)                  # smax(0.0, c/dd)
        u = np.where(dd > 0.0, np.where(lo < 1.0, lo, 1.0), 0.0)  # smin(1.0, .)
        rx, ry = wx - u * dx, wy - u * dy
        D = rx * rx + ry * ry
        nan = np.isnan(D)
        win = np.lexsort((i, np.where(nan, 0.0, D), nan))[0]    # least (isnan(D), D, i)
        if nan[win]:
            return None
        i0, u0, D0 = int(i[win]), u[win], D[win]
        root = np.sqrt(D0)
        t0 = t[i0] + u0 * (t[i0 + 1] - t[i0])
        e = -root if dx[win] * wy[win] - dy[win] * wx[win] < 0.0 else root
        return i0, u0, D0, e, t0, (np.float64(i0) + u0) * hb


def _hzn_wrap(tau, T, closed: bool):
    """(lap, w): the horizon stage's wrap count and row time of the tick times tau."""
    if not closed:
        return np.zeros(tau.shape[0]), tau
    with np.errstate(all="ignore"):
        lap = np.floor(tau / T)
        w = tau - lap * T
        neg = w < 0.0
        over = ~neg & (w >= T)
        return (np.where(neg, lap - 1.0, np.where(over, lap + 1.0, lap)),
                np.where(neg, w + T, np.where(over, w - T, w)))


def _hzn_segment(t, S: int, w):
    """The segments of the row times w: the trajectory stage's bisection over the stamps t[0..S]."""
    return np.clip(np.searchsorted(t[:S + 1], w, side="right") - 1, 0, S - 1)


def _hzn_columns(row6, t, hb, closed: bool, lap, w) -> tuple:
    """The horizon stage's seven columns (TRAJ_COLS' order) at the row times w in the laps lap."""
    X, Y, PSI, K, V, A = row6
    N = X.shape[0]
    S = N if closed else N - 1
    with np.errstate(all="ignore"):
        i = _hzn_segment(t, S, w)
        j = (i + 1) % N
        um = (w - t[i]) / (t[i + 1] - t[i])
        d = PSI[j] - PSI[i]
        d = np.where(d > np.pi, d - 2.0 * np.pi, np.where(d < -np.pi, d + 2.0 * np.pi, d))
        return (((lap * np.float64(S) + i.astype(np.float64)) + um) * hb, X[i] + um * (X[j] - X[i]),
                Y[i] + um * (Y[j] - Y[i]), PSI[i] + um * d, K[i] + um * (K[j] - K[i]), V[i] + um * (V[j] - V[i]), A[i])


def horizon_host(x, y, heading, kappa, v, ax, h, closed: bool, poses, row=None, seg_hint=None, window: int = 0,
                 dt: float = 0.05, m_cap: int = 64, stamps=None) -> Horizon:
    """The specification of the horizon stage (include/rl_abi.h) in NumPy; the kernel
    equals it bit for bit.  Rows [B, N] (or one row [N]) with steps h as for trajectory_host,
    whose stamps they get unless `stamps` [B, N + 1] gives them (a plan's, as fetched).  Pose q
    [Q, 2] is located on row[q] (None: row 0) among all S segments (seg_hint None or -1) or the
    segments within `window` of seg_hint[q], around the start line on a closed row; the winner
    is the least (isnan(D), D, i).  Then up to m_cap ticks at t0 + m * dt: open rows stop
    before T, closed rows wrap modulo T and count the laps in s."""
    closed = bool(closed)
    rows, hs, stamps, N, S, (P, rw, hint) = _query_rows(
        "horizon", (x, y, heading, kappa, v, ax, h), closed, lambda: _hzn_query(poses, row, seg_hint, window, dt, m_cap),
        stamps)
    Q, dt, m_cap, W = P.shape[0], float(dt), int(m_cap), int(window)
    out = Horizon.alloc(Q, m_cap, dt)
    out.seg[:] = -1
    steps = np.arange(m_cap, dtype=np.float64)
    for k in range(Q):
        if S < 1:
            continue
        row6 = [a[rw[k]] for a in rows]
        t, hb = stamps[rw[k]], hs[rw[k]]
        T = t[S]
        loc = _hzn_locate(row6[0], row6[1], t, hb, P[k, 0], P[k, 1], int(hint[k]), W, closed)
        if loc is None:
            continue
        out.seg[k], out.u[k], out.dist2[k], out.e[k], out.t0[k], out.s0[k] = loc
        with np.errstate(all="ignore"):
            tau = out.t0[k] + steps * dt
            lap, w = _hzn_wrap(tau, T, closed)
            if closed:
                M = m_cap if np.isfinite(T) and T > 0.0 else 0
            else:
                M = int(np.count_nonzero(tau < T))                  # (monotone in m: the kernel bisects)
            out.count[k] = M
            if M == 0:
                continue
            for n, col in zip(abi.TRAJ_COLS, _hzn_columns(row6, t, hb, closed, lap[:M], w[:M])):
                getattr(out, n)[k, :M] = col
    return out


def horizon(x, y, heading, kappa, v, ax, h, closed: bool, poses, row=None, seg_hint=None, window: int = 0,
            dt: float = 0.05, m_cap: int = 64, device: int = 0) -> Horizon:
    """horizon_host on the GPU (rl_horizon): the trajectory kernel stamps the B given rows, then
    the horizon kernel answers the Q poses; row[q] counts the given rows."""
    rows, hs, (P, rw, hint), B, N = _open_query("horizon", (x, y, heading, kappa, v, ax, h),
                                                lambda: _hzn_query(poses, row, seg_hint, window, dt, m_cap))
    return _one_shot("rl_horizon", rows, hs, N, B, closed, _hzn_c(P, rw, hint, window, dt, m_cap),
                     Horizon.alloc(P.shape[0], int(m_cap), dt), device)


# ------------------------------------------------- rejoin: a reachable profile from the car's speed
class _FromTheCar(Horizon):
    """Horizon whose ticks are counted from the car (the rejoin and stop stages' answers)."""

    def row(self, q: int) -> dict:
        """The ticks of query q: t [count[q]] = m * dt, from the car, and the seven columns."""
        m = int(self.count[q])
        out = {"t": np.arange(m, dtype=np.float64) * self.dt}
        for n in abi.TRAJ_COLS:
            out[n] = getattr(self, n)[q, :m]
        return out


@dataclass
class Rejoin(_FromTheCar):
    """The rejoin stage's answer for Q poses (rl_rjn): Horizon's fields, with the ticks counted
    from the car (t = m * dt) along the reachable speed profile, and merge_node (the march node
    at which the profile meets the row's, -1: not within k_cap nodes or the row's end),
    overspeed (nodes at which the car is faster than the row), t_merge (the time marched),
    t_loss (the time lost against the row's own schedule, NaN when not merged) [Q]; node_v,
    node_t [Q, k_cap + 1]: the march's speeds and times, the entries after node_end(q)
    unspecified."""

    merge_node: np.ndarray = None
    overspeed: np.ndarray = None
    t_merge: np.ndarray = None
    t_loss: np.ndarray = None
    node_v: np.ndarray = None
    node_t: np.ndarray = None
    k_lim: np.ndarray = None      # [Q] nodes the march may take (host side: from seg, N and closed)

    _C = abi.RlRjn
    _PER = abi.HZN_LOC + abi.RJN_SCAL
    _INTS = abi.RJN_INTS
    _NODES = abi.RJN_NODES
    _HOST_INTS = ("k_lim",)

    def set_k_lim(self, N: int, closed: bool) -> None:
        room = np.full(self.seg.shape, N) if closed else N - 1 - self.seg
        self.k_lim = np.where(self.seg >= 0, np.minimum(self.node_v.shape[1] - 1, room), 0).astype(np.int32)

    def node_end(self, q: int) -> int:
        """K_end: the last march node of query q (the merge node, or the last node marched)."""
        return int(self.merge_node[q]) if self.merge_node[q] >= 0 else int(self.k_lim[q])


def _rjn_query(poses, v0, cfg, row, seg_hint, window, dt, m_cap, k_cap) -> tuple:
    P, rw, hint = _hzn_query(poses, row, seg_hint, window, dt, m_cap)
    Q = P.shape[0]
    V0 = np.asarray(v0, dtype=np.float64)
    if V0.ndim == 0:
        V0 = np.broadcast_to(V0, (Q,))
    if V0.shape != (Q,):
        raise ValueError(f"rejoin: v0 must be a number or [Q={Q}] numbers, got shape {V0.shape}")
    V0 = np.ascontiguousarray(V0)
    if not np.all(np.isfinite(V0)) or np.any(V0 < 0.0):
        raise ValueError("rejoin: v0 must be finite and >= 0")
    if not isinstance(cfg, RlCfg):
        raise ValueError("rejoin: cfg must be one RlCfg (the car's limits now)")
    if int(k_cap) != k_cap or not 1 <= int(k_cap) <= abi.RL_RJN_MAX_NODES:
        raise ValueError(f"rejoin: k_cap must be 1..{abi.RL_RJN_MAX_NODES}, got {k_cap}")
    return P, rw, hint, V0


def _rjn_c(P, rw, hint, V0, cfg, window, dt, m_cap, k_cap) -> abi.RlRjnQuery:
    hq = _hzn_c(P, rw, hint, window, dt, m_cap)
    return abi.RlRjnQuery(*[getattr(hq, n) for n, _ in abi.RlHznQuery._fields_], _ptr(V0, np.float64, "v0"), C.pointer(cfg),
                          int(k_cap), 0)


def _smax(a: float, b: float) -> float:
    return b if a < b else a


def _smin(a: float, b: float) -> float:
    return b if b < a else a


def _fdiv(a: float, b: float) -> float:
    """IEEE a / b (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _ax_max_at(c: tuple, vi: float, ki: float) -> tuple:
    """(a_acc, a_brk): the reference's ax_max_at (ref:797-824) with its constant prefixes c."""
    a_total2, kFd, Fr, mass, Pmax, acc_cap, brk_cap = c
    alat = vi * vi * abs(ki)
    a_res = math.sqrt(_smax(0.0, a_total2 - alat * alat))
    Fd = kFd * vi * vi
    a_power = (_fdiv(Pmax, mass * vi) - _fdiv(Fd + Fr, mass)) if (Pmax > 0 and vi > 1e-6) else 1e9
    a_acc = _smax(0.0, _smin(_smin(a_res, acc_cap), a_power))
    a_brk = _smax(0.0, _smin(a_res, brk_cap) + _fdiv(Fd + Fr, mass))
    return a_acc, a_brk


def _rjn_consts(cfg: RlCfg) -> tuple:
    a_total = _smax(cfg.a_total_max, cfg.a_lat_max) if cfg.use_total_ge_lat else cfg.a_total_max
    return (a_total * a_total, 0.5 * cfg.rho_air * cfg.Cd * cfg.A_front_m2, cfg.mass_kg * 9.81 * cfg.c_rr,
            cfg.mass_kg, cfg.P_max_W, cfg.a_long_acc_cap, cfg.a_long_brake_cap)


def _bisect_nodes(tt: np.ndarray, tau: np.ndarray, hi: int) -> np.ndarray:
    """The kernel's bisection for every tau: a = 0, e = hi; while e - a > 1: mid = a + (e - a) // 2;
    tt[mid] <= tau ? a = mid : e = mid."""
    a = np.zeros(tau.shape[0], dtype=np.int64)
    e = np.full(tau.shape[0], hi, dtype=np.int64)
    while np.any(e - a > 1):
        go = e - a > 1
        mid = a + ((e - a) >> 1)
        le = tt[mid] <= tau
        a = np.where(go & le, mid, a)
        e = np.where(go & ~le, mid, e)
    return a


def _march_nodes(row6, i0: int, u: float, hb: float, K: int) -> tuple:
    """The march nodes 0 .. K of a point located on segment i0 at u: (n, idx, kap, r, d0), the
    nodes' samples unwrapped and as row indices, their curvatures and the row's speeds there
    (node 0: interpolated with u) and node 0's distance to node 1."""
    KAP, V = row6[3], row6[4]
    N = KAP.shape[0]
    j0 = (i0 + 1) % N
    n = i0 + np.arange(K + 1)
    idx = n % N
    with np.errstate(all="ignore"):
        kap = KAP[idx].copy()
        r = V[idx].copy()
        kap[0] = KAP[i0] + u * (KAP[j0] - KAP[i0])
        r[0] = V[i0] + u * (V[j0] - V[i0])
        d0 = (1.0 - u) * hb
    return n, idx, kap, r, d0


def _march_step(consts: tuple, wk: float, kap_k: float, d: float) -> tuple:
    """(up, dn): the fastest and the slowest speed at the next node, from wk over the distance d
    (the device's march_step)."""
    a_acc, a_brk = _ax_max_at(consts, wk, kap_k)
    return math.sqrt(_smax(0.0, wk * wk + (2.0 * a_acc) * d)), math.sqrt(_smax(0.0, wk * wk - (2.0 * a_brk) * d))


def _node_values(row6, nodes, i0: int, u: float, hb: float, s0) -> tuple:
    """(x, y, psi, s) of the march nodes, nodes = _march_nodes': node 0 the located point (s0 its
    arc length), node k >= 1 sample n_k (the device's march_node)."""
    X, Y, PSI = row6[:3]
    n, idx = nodes[:2]
    j0 = (i0 + 1) % X.shape[0]
    dp0 = PSI[j0] - PSI[i0]
    dp0 = dp0 - 2.0 * np.pi if dp0 > np.pi else (dp0 + 2.0 * np.pi if dp0 < -np.pi else dp0)
    nx, ny, npsi = X[idx].copy(), Y[idx].copy(), PSI[idx].copy()
    ns = n.astype(np.float64) * hb
    nx[0] = X[i0] + u * (X[j0] - X[i0])
    ny[0] = Y[i0] + u * (Y[j0] - Y[i0])
    npsi[0] = PSI[i0] + u * dp0
    ns[0] = s0
    return nx, ny, npsi, ns


def _node_ticks(out, q: int, M1: int, tau, tt, w, kend: int, values, kap, d) -> np.ndarray:
    """The seven columns of the ticks tau[:M1] of query q on the march w, tt over the nodes
    0 .. kend with values = (x, y, psi, s), curvatures kap and d [kend] apart (the device's
    march_columns).  Returns the ticks' nodes a and parameters um [2, M1]."""
    nx, ny, npsi, ns = values
    a = _bisect_nodes(tt, tau, kend)
    b = a + 1
    um = (tau - tt[a]) / (tt[b] - tt[a])
    d = d[a]
    dp = npsi[b] - npsi[a]
    dp = np.where(dp > np.pi, dp - 2.0 * np.pi, np.where(dp < -np.pi, dp + 2.0 * np.pi, dp))
    out.s[q, :M1] = ns[a] + um * (ns[b] - ns[a])
    out.x[q, :M1] = nx[a] + um * (nx[b] - nx[a])
    out.y[q, :M1] = ny[a] + um * (ny[b] - ny[a])
    out.heading[q, :M1] = npsi[a] + um * dp
    out.kappa[q, :M1] = kap[a] + um * (kap[b] - kap[a])
    out.v[q, :M1] = w[a] + um * (w[b] - w[a])
    out.ax[q, :M1] = np.where(d > 0.0, (w[b] * w[b] - w[a] * w[a]) / (2.0 * d), 0.0)
    return a, um


def _march_ticks(out, q: int, M1: int, tau, tt, w, kend: int, row6, nodes, i0: int, u: float, hb: float) -> None:
    """The seven columns of the ticks tau[:M1] of query q on the march w, tt over the nodes
    0 .. kend, nodes = _march_nodes' (the device's march_columns)."""
    kap, d0 = nodes[2], nodes[4]
    d = np.concatenate(([d0], np.full(max(kend - 1, 0), hb)))
    _node_ticks(out, q, M1, tau, tt, w, kend, _node_values(row6, nodes, i0, u, hb, out.s0[q]), kap, d)


def rejoin_host(x, y, heading, kappa, v, ax, h, closed: bool, poses, v0, cfg: RlCfg, row=None, seg_hint=None,
                window: int = 0, dt: float = 0.05, m_cap: int = 64, k_cap: int = 1024, stamps=None) -> Rejoin:
    """The specification of the rejoin stage (include/rl_abi.h) in NumPy; the kernel
    equals it bit for bit.  The rows, poses, hints and stamps are horizon_host's, and so is the
    locate.  v0 (a number or [Q]) is the car's speed and cfg its limits now.  From the located
    point the reachable speed nearest the row's is marched node by node (the samples ahead, at
    most k_cap) until it equals the row's; the ticks m * dt, counted from the car, follow the
    marched profile and then the row's own from the merge on."""
    closed = bool(closed)
    rows, hs, stamps, N, S, (P, rw, hint, V0) = _query_rows(
        "rejoin", (x, y, heading, kappa, v, ax, h), closed,
        lambda: _rjn_query(poses, v0, cfg, row, seg_hint, window, dt, m_cap, k_cap), stamps)
    Q, dt, m_cap, W, k_cap = P.shape[0], float(dt), int(m_cap), int(window), int(k_cap)
    consts = _rjn_consts(cfg)
    out = Rejoin.alloc(Q, m_cap, dt, k_cap)
    out.seg[:] = -1
    out.merge_node[:] = -1
    tau_all = np.arange(m_cap, dtype=np.float64) * dt
    for q in range(Q):
        if S < 1:
            continue
        row6 = [a[rw[q]] for a in rows]
        t, hb = stamps[rw[q]], float(hs[rw[q]])
        T = t[S]
        loc = _hzn_locate(row6[0], row6[1], t, hb, P[q, 0], P[q, 1], int(hint[q]), W, closed)
        if loc is None:
            continue
        out.seg[q], out.u[q], out.dist2[q], out.e[q], out.t0[q], out.s0[q] = loc
        i0, u, t0 = int(loc[0]), float(loc[1]), float(loc[4])
        K_lim = min(k_cap, N if closed else N - 1 - i0)
        out.k_lim[q] = K_lim
        nodes = _, _, kap, r, d0 = _march_nodes(row6, i0, u, hb, K_lim)
        kl, rl_, w, tt = kap.tolist(), r.tolist(), [float(V0[q])], [0.0]
        ks, over = -1, 0
        if w[0] == rl_[0]:
            ks = 0
        else:
            over += w[0] > rl_[0]
            for k in range(K_lim):
                d, wk = (d0 if k == 0 else hb), w[k]
                up, dn = _march_step(consts, wk, kl[k], d)
                wn = _smin(up, _smax(dn, rl_[k + 1]))
                w.append(wn)
                tt.append(tt[k] + _fdiv(2.0 * d, _smax(1e-6, wk + wn)))
                if wn == rl_[k + 1]:
                    ks = k + 1
                    break
                over += wn > rl_[k + 1]
        kend = ks if ks >= 0 else K_lim
        w, tt = np.array(w), np.array(tt)
        out.node_v[q, :kend + 1], out.node_t[q, :kend + 1] = w, tt
        tte = tt[kend]
        nk = i0 + max(ks, 0)
        c0 = nk // N
        tref = t0 if ks == 0 else t[nk - c0 * N]
        out.merge_node[q], out.overspeed[q], out.t_merge[q] = ks, over, tte
        with np.errstate(all="ignore"):
            out.t_loss[q] = tte - ((np.float64(c0) * T + tref) - t0) if ks >= 0 else np.nan
            M1 = int(np.count_nonzero(tau_all < tte))           # (monotone in m: the kernel bisects)
            wref = tref + (tau_all - tte)
            if ks < 0:
                M = M1
            elif closed:
                M = m_cap if np.isfinite(T) and T > 0.0 else M1
            else:
                M = M1 + int(np.count_nonzero(wref[M1:] < T))
            out.count[q] = M
            if M1 > 0:
                _march_ticks(out, q, M1, tau_all[:M1], tt, w, kend, row6, nodes, i0, u, hb)
            if M > M1:
                lap, wr = _hzn_wrap(wref[M1:M], T, closed)
                for name, col in zip(abi.TRAJ_COLS, _hzn_columns(row6, t, hb, closed, np.float64(c0) + lap, wr)):
                    getattr(out, name)[q, M1:M] = col
    return out


def rejoin(x, y, heading, kappa, v, ax, h, closed: bool, poses, v0, cfg: RlCfg, row=None, seg_hint=None,
           window: int = 0, dt: float = 0.05, m_cap: int = 64, k_cap: int = 1024, device: int = 0) -> Rejoin:
    """rejoin_host on the GPU (rl_rejoin): the trajectory kernel stamps the B given rows, then the
    rejoin kernel answers the Q poses; row[q] counts the given rows."""
    rows, hs, (P, rw, hint, V0), B, N = _open_query(
        "rejoin", (x, y, heading, kappa, v, ax, h), lambda: _rjn_query(poses, v0, cfg, row, seg_hint, window, dt, m_cap, k_cap))
    out = _one_shot("rl_rejoin", rows, hs, N, B, closed, _rjn_c(P, rw, hint, V0, cfg, window, dt, m_cap, k_cap),
                    Rejoin.alloc(P.shape[0], int(m_cap), dt, int(k_cap)), device)
    out.set_k_lim(N, bool(closed))
    return out


# ------------------------------------------------- stop: brake to a target speed at a sample
@dataclass
class Stop(_FromTheCar):
    """The stop stage's answer for Q poses (rl_stp): Horizon's fields, with the ticks counted from
    the car (t = m * dt) along the march up to the target, and stop_node (the march node of the
    target sample, -1: the target is not among the nodes ahead), reachable (1: the car is inside
    the brake envelope and meets the target), overspeed (nodes at which the car is faster than
    the lower of the envelope and the row), brake_node (the first node at which the envelope is
    below the row's speed), t_stop, v_end (the time and the speed at the target), s_stop (its arc
    length), v_excess (the largest excess over the lower of the envelope and the row) [Q];
    node_v, node_t, node_b [Q, k_cap + 1]: the march's speeds and times and the envelope, the
    entries after node_end(q) unspecified.  Where stop_node is -1 only seg, count and the
    location are specified."""

    stop_node: np.ndarray = None
    overspeed: np.ndarray = None
    reachable: np.ndarray = None
    brake_node: np.ndarray = None
    t_stop: np.ndarray = None
    v_end: np.ndarray = None
    s_stop: np.ndarray = None
    v_excess: np.ndarray = None
    node_v: np.ndarray = None
    node_t: np.ndarray = None
    node_b: np.ndarray = None

    _C = abi.RlStp
    _PER = abi.HZN_LOC + abi.STP_SCAL
    _INTS = abi.STP_INTS
    _NODES = abi.STP_NODES

    def node_end(self, q: int) -> int:
        """K_s: the target's march node of query q (-1: out of range)."""
        return int(self.stop_node[q])


def _stp_query(poses, v0, cfg, stop_sample, v_target, row, seg_hint, window, dt, m_cap, k_cap) -> tuple:
    P, rw, hint, V0 = _rjn_query(poses, v0, cfg, row, seg_hint, window, dt, m_cap, k_cap)
    Q = P.shape[0]
    if stop_sample is None:
        raise ValueError("stop: stop_sample is None")
    J = np.asarray(stop_sample)
    if J.ndim == 0:
        J = np.broadcast_to(J, (Q,))
    if J.shape != (Q,) or not np.issubdtype(J.dtype, np.integer):
        raise ValueError(f"stop: stop_sample must be an integer or [Q={Q}] integers, got {J.dtype} {J.shape}")
    J = np.ascontiguousarray(J, dtype=np.int32)
    VT = np.asarray(0.0 if v_target is None else v_target, dtype=np.float64)
    if VT.ndim == 0:
        VT = np.broadcast_to(VT, (Q,))
    if VT.shape != (Q,):
        raise ValueError(f"stop: v_target must be a number or [Q={Q}] numbers, got shape {VT.shape}")
    VT = np.ascontiguousarray(VT)
    if not np.all(np.isfinite(VT)) or np.any(VT < 0.0):
        raise ValueError("stop: v_target must be finite and >= 0")
    return P, rw, hint, V0, J, VT


def _stp_c(P, rw, hint, V0, cfg, J, VT, window, dt, m_cap, k_cap) -> abi.RlStpQuery:
    """VT None: a NULL v_target, all 0.0."""
    return abi.RlStpQuery(_rjn_c(P, rw, hint, V0, cfg, window, dt, m_cap, k_cap), _ptr(J, np.int32, "stop_sample"),
                          None if VT is None else _ptr(VT, np.float64, "v_target"))


def stop_host(x, y, heading, kappa, v, ax, h, closed: bool, poses, v0, cfg: RlCfg, stop_sample, v_target=None,
              row=None, seg_hint=None, window: int = 0, dt: float = 0.05, m_cap: int = 64, k_cap: int = 1024,
              stamps=None) -> Stop:
    """The specification of the stop stage (include/rl_abi.h) in NumPy; the kernel
    equals it bit for bit.  The rows, poses, hints, stamps, v0 and cfg are rejoin_host's, and so
    are the locate and the nodes.  stop_sample (an integer or [Q]) is the row sample at which the
    car must do v_target (a number or [Q]; None: 0.0): its node K_s is the first time that
    sample comes up ahead of the located segment.  A brake envelope b is swept backward from
    b[K_s] = v_target with cfg, v0 is marched forward to K_s under it (inside the envelope the
    envelope caps the speed, outside it the car brakes as hard as cfg allows), and the ticks
    m * dt before t_stop follow the march."""
    def in_row(N, qy):
        _P, _rw, _hint, _V0, J, _VT = qy
        if np.any(J < 0) or np.any(J >= N):
            raise ValueError(f"stop: stop_sample outside [0, {N})")

    closed = bool(closed)
    rows, hs, stamps, N, S, (P, rw, hint, V0, J, VT) = _query_rows(
        "stop", (x, y, heading, kappa, v, ax, h), closed,
        lambda: _stp_query(poses, v0, cfg, stop_sample, v_target, row, seg_hint, window, dt, m_cap, k_cap), stamps, in_row)
    Q, dt, m_cap, W, k_cap = P.shape[0], float(dt), int(m_cap), int(window), int(k_cap)
    consts = _rjn_consts(cfg)
    out = Stop.alloc(Q, m_cap, dt, k_cap)
    out.seg[:] = -1
    out.stop_node[:] = -1
    tau_all = np.arange(m_cap, dtype=np.float64) * dt
    for q in range(Q):
        if S < 1:
            continue
        row6 = [a[rw[q]] for a in rows]
        t, hb = stamps[rw[q]], float(hs[rw[q]])
        loc = _hzn_locate(row6[0], row6[1], t, hb, P[q, 0], P[q, 1], int(hint[q]), W, closed)
        if loc is None:
            continue
        out.seg[q], out.u[q], out.dist2[q], out.e[q], out.t0[q], out.s0[q] = loc
        i0, u = int(loc[0]), float(loc[1])
        K_lim = min(k_cap, N if closed else N - 1 - i0)
        Ks = (int(J[q]) - i0 - 1) % N + 1 if closed else int(J[q]) - i0
        if Ks < 1 or Ks > K_lim:
            continue
        nodes = _, _, kap, r, d0 = _march_nodes(row6, i0, u, hb, Ks)
        kl, rl_ = kap.tolist(), r.tolist()
        b = [0.0] * (Ks + 1)                                # the envelope, backward from the target
        b[Ks] = float(VT[q])
        for k in range(Ks - 1, -1, -1):
            d, bn = (d0 if k == 0 else hb), b[k + 1]
            a_brk = _ax_max_at(consts, bn, kl[k + 1])[1]
            b[k] = math.sqrt(_smax(0.0, bn * bn + (2.0 * a_brk) * d))
        w, tt = [float(V0[q])], [0.0]                       # the march, forward to the target
        over, ve, brake = 0, 0.0, -1
        for k in range(Ks + 1):
            wk = w[k]
            g = _smin(b[k], rl_[k])
            over += wk > g
            ve = _smax(ve, wk - g)
            if brake < 0 and b[k] < rl_[k]:
                brake = k
            if k == Ks:
                break
            d = d0 if k == 0 else hb
            up, dn = _march_step(consts, wk, kl[k], d)
            if wk <= b[k]:
                wn = _smin(up, _smin(b[k + 1], _smax(dn, rl_[k + 1])))
            else:
                wn = _smin(up, _smax(dn, _smin(b[k + 1], rl_[k + 1])))
            w.append(wn)
            tt.append(tt[k] + _fdiv(2.0 * d, _smax(1e-6, wk + wn)))
        reach = float(V0[q]) <= b[0]
        w, tt, b = np.array(w), np.array(tt), np.array(b)
        out.node_v[q, :Ks + 1], out.node_t[q, :Ks + 1], out.node_b[q, :Ks + 1] = w, tt, b
        tte = tt[Ks]
        out.stop_node[q], out.overspeed[q], out.reachable[q] = Ks, over, 1 if reach else 0
        out.brake_node[q] = Ks if brake < 0 else brake
        out.t_stop[q], out.v_end[q], out.v_excess[q] = tte, w[Ks], ve
        with np.errstate(all="ignore"):
            out.s_stop[q] = np.float64(i0 + Ks) * hb
            M1 = int(np.count_nonzero(tau_all < tte))           # (monotone in m: the kernel bisects)
            out.count[q] = M1
            if M1 > 0:
                _march_ticks(out, q, M1, tau_all[:M1], tt, w, Ks, row6, nodes, i0, u, hb)
    return out


def stop(x, y, heading, kappa, v, ax, h, closed: bool, poses, v0, cfg: RlCfg, stop_sample, v_target=None, row=None,
         seg_hint=None, window: int = 0, dt: float = 0.05, m_cap: int = 64, k_cap: int = 1024, device: int = 0) -> Stop:
    """stop_host on the GPU (rl_stop): the trajectory kernel stamps the B given rows, then the
    stop kernel answers the Q poses; row[q] counts the given rows."""
    rows, hs, (P, rw, hint, V0, J, VT), B, N = _open_query(
        "stop", (x, y, heading, kappa, v, ax, h),
        lambda: _stp_query(poses, v0, cfg, stop_sample, v_target, row, seg_hint, window, dt, m_cap, k_cap))
    qc = _stp_c(P, rw, hint, V0, cfg, J, None if v_target is None else VT, window, dt, m_cap, k_cap)
    return _one_shot("rl_stop", rows, hs, N, B, closed, qc, Stop.alloc(P.shape[0], int(m_cap), dt, int(k_cap)), device)


# ------------------------------------------------- retime: the speed profile under the car's limits now
@dataclass
class Retime(_FromTheCar):
    """The retime stage's answer for Q poses (rl_rtm): Horizon's fields, with the ticks counted from
    the car (t = m * dt) along the march over the nodes ahead, and end_node (the last node K, -1:
    no answer), feasible (1: the car is inside the envelope of cfg), overspeed (nodes at which the
    car is faster than the envelope), bind_node (the first node at which the envelope is below the
    row's speed, -1: none), t_end (the time marched), t_loss (the time lost against the row's own
    schedule over the window), v_excess (the largest excess over the envelope) [Q]; node_v, node_t,
    node_b, node_c [Q, k_cap + 1]: the march's speeds and times, the envelope and the ceiling, the
    entries after node_end(q) unspecified.  Where end_node is -1 only seg and count are specified."""

    end_node: np.ndarray = None
    overspeed: np.ndarray = None
    feasible: np.ndarray = None
    bind_node: np.ndarray = None
    t_end: np.ndarray = None
    t_loss: np.ndarray = None
    v_excess: np.ndarray = None
    node_v: np.ndarray = None
    node_t: np.ndarray = None
    node_b: np.ndarray = None
    node_c: np.ndarray = None

    _C = abi.RlRtm
    _PER = abi.HZN_LOC + abi.RTM_SCAL
    _INTS = abi.RTM_INTS
    _NODES = abi.RTM_NODES

    def node_end(self, q: int) -> int:
        """K: the last march node of query q (-1: no answer)."""
        return int(self.end_node[q])


def _retime_pass(consts: tuple, cfg: RlCfg, v0: float, kap, r, d) -> tuple:
    """The retime stage's ceiling, envelope and march over the nodes 0 .. K of curvatures kap and
    row speeds r [K + 1], d [K] apart, from v0: (w, tt, b, c [K + 1], overspeed, v_excess,
    bind_node) (the device's retime_ceiling and retime_pass)."""
    v_cap, a_lat, k_eps = float(cfg.v_cap_mps), float(cfg.a_lat_max), float(cfg.kappa_eps)
    kl, rl_, K = np.asarray(kap).tolist(), np.asarray(r).tolist(), len(d)
    c = [_smin(_smin(v_cap, math.sqrt(_fdiv(a_lat, _smax(abs(kk), k_eps)))), rk)     # the ceiling, per node
         for kk, rk in zip(kl, rl_)]
    b = [0.0] * (K + 1)                                 # the envelope, backward from the last node
    b[K] = c[K]
    for k in range(K - 1, -1, -1):
        bn = b[k + 1]
        a_brk = _ax_max_at(consts, bn, kl[k + 1])[1]
        b[k] = _smin(c[k], math.sqrt(_smax(0.0, bn * bn + (2.0 * a_brk) * d[k])))
    w, tt = [v0], [0.0]                                 # the march, forward to the last node
    over, ve, bind = 0, 0.0, -1
    for k in range(K + 1):
        wk = w[k]
        over += wk > b[k]
        ve = _smax(ve, wk - b[k])
        if bind < 0 and b[k] < rl_[k]:
            bind = k
        if k == K:
            break
        up, dn = _march_step(consts, wk, kl[k], d[k])
        wn = _smin(up, b[k + 1] if wk <= b[k] else _smax(dn, b[k + 1]))
        w.append(wn)
        tt.append(tt[k] + _fdiv(2.0 * d[k], _smax(1e-6, wk + wn)))
    return np.array(w), np.array(tt), np.array(b), np.array(c), over, ve, bind


def retime_host(x, y, heading, kappa, v, ax, h, closed: bool, poses, v0, cfg: RlCfg, row=None, seg_hint=None,
                window: int = 0, dt: float = 0.05, m_cap: int = 64, k_cap: int = 1024, stamps=None) -> Retime:
    """The specification of the retime stage (include/rl_abi.h) in NumPy; the kernel
    equals it bit for bit.  The rows, poses, hints, stamps, v0 and cfg are rejoin_host's, and so
    are the locate and the nodes 0 .. K = K_lim.  Per node the ceiling c is the lowest of cfg's
    v_cap, its lateral limit sqrt(a_lat_max / |kappa|) and the row's speed r; the envelope b is
    swept backward under c from b[K] = c[K] with cfg's braking; v0 is marched forward to K under b
    (inside the envelope the envelope caps the speed, outside it the car brakes as hard as cfg
    allows); and the ticks m * dt before t_end follow the march.  It is the reference's
    velocity_profile_forward_backward over the nodes ahead, with the car's cfg, from the car's
    speed."""
    closed = bool(closed)
    rows, hs, stamps, N, S, (P, rw, hint, V0) = _query_rows(
        "retime", (x, y, heading, kappa, v, ax, h), closed,
        lambda: _rjn_query(poses, v0, cfg, row, seg_hint, window, dt, m_cap, k_cap), stamps)
    Q, dt, m_cap, W, k_cap = P.shape[0], float(dt), int(m_cap), int(window), int(k_cap)
    consts = _rjn_consts(cfg)
    out = Retime.alloc(Q, m_cap, dt, k_cap)
    out.seg[:] = -1
    out.end_node[:] = -1
    tau_all = np.arange(m_cap, dtype=np.float64) * dt
    for q in range(Q):
        if S < 1:
            continue
        row6 = [a[rw[q]] for a in rows]
        t, hb = stamps[rw[q]], float(hs[rw[q]])
        T = t[S]
        loc = _hzn_locate(row6[0], row6[1], t, hb, P[q, 0], P[q, 1], int(hint[q]), W, closed)
        if loc is None:
            continue
        i0, u, t0 = int(loc[0]), float(loc[1]), loc[4]
        K = min(k_cap, N if closed else N - 1 - i0)
        if K < 1:
            continue
        out.seg[q], out.u[q], out.dist2[q], out.e[q], out.t0[q], out.s0[q] = loc
        nodes = _, _, kap, r, d0 = _march_nodes(row6, i0, u, hb, K)
        w, tt, b, c, over, ve, bind = _retime_pass(consts, cfg, float(V0[q]), kap, r, [d0] + [hb] * (K - 1))
        out.node_v[q, :K + 1], out.node_t[q, :K + 1], out.node_b[q, :K + 1], out.node_c[q, :K + 1] = w, tt, b, c
        tte = tt[K]
        out.end_node[q], out.overspeed[q], out.feasible[q] = K, over, 1 if float(V0[q]) <= b[0] else 0
        out.bind_node[q], out.t_end[q], out.v_excess[q] = bind, tte, ve
        nk = i0 + K
        c0 = nk // N
        with np.errstate(all="ignore"):
            out.t_loss[q] = tte - ((np.float64(c0) * T + t[nk - c0 * N]) - t0)
            M1 = int(np.count_nonzero(tau_all < tte))           # (monotone in m: the kernel bisects)
            out.count[q] = M1
            if M1 > 0:
                _march_ticks(out, q, M1, tau_all[:M1], tt, w, K, row6, nodes, i0, u, hb)
    return out


def _rtm_c(P, rw, hint, V0, cfg, window, dt, m_cap, k_cap) -> abi.RlRtmQuery:
    return abi.RlRtmQuery(_rjn_c(P, rw, hint, V0, cfg, window, dt, m_cap, k_cap))


def retime(x, y, heading, kappa, v, ax, h, closed: bool, poses, v0, cfg: RlCfg, row=None, seg_hint=None,
           window: int = 0, dt: float = 0.05, m_cap: int = 64, k_cap: int = 1024, device: int = 0) -> Retime:
    """retime_host on the GPU (rl_retime): the trajectory kernel stamps the B given rows, then the
    retime kernel answers the Q poses; row[q] counts the given rows."""
    rows, hs, (P, rw, hint, V0), B, N = _open_query(
        "retime", (x, y, heading, kappa, v, ax, h), lambda: _rjn_query(poses, v0, cfg, row, seg_hint, window, dt, m_cap, k_cap))
    return _one_shot("rl_retime", rows, hs, N, B, closed, _rtm_c(P, rw, hint, V0, cfg, window, dt, m_cap, k_cap),
                     Retime.alloc(P.shape[0], int(m_cap), dt, int(k_cap)), device)


# ------------------------------------------------- bounds: the free track width along the rows
@dataclass
class Bounds:
    """The bounds stage's rows (rl_bnd), [R, N] each: the lateral room lo <= 0 <= hi about every
    sample along its unit normal (nx, ny), +n left of travel (the sign of Horizon.e)."""

    lo: np.ndarray
    hi: np.ndarray
    nx: np.ndarray
    ny: np.ndarray

    _C, _NODES = abi.RlBnd, ()          # (Plan._stage_fetch)

    @classmethod
    def alloc(cls, R: int, N: int) -> "Bounds":
        return cls(*[np.zeros((R, N)) for _ in abi.BND_ROWS])

    def as_c(self) -> abi.RlBnd:
        return abi.RlBnd(*[_ptr(getattr(self, n), np.float64, n) for n in abi.BND_ROWS])


@dataclass
class HorizonBounds:
    """The bounds at the horizon stage's ticks (rl_hzn_bnd): lo, hi [Q, M_cap], of which the first
    Horizon.count[q] of query q are specified, and lo0, hi0 [Q] at the located segment: with
    Horizon.e the room now is hi0 - e on the left and e - lo0 on the right.  A query with
    seg = -1 has nothing specified."""

    lo: np.ndarray
    hi: np.ndarray
    lo0: np.ndarray
    hi0: np.ndarray

    _C, _NODES = abi.RlHznBnd, ()          # (Plan._stage_fetch)

    @classmethod
    def alloc(cls, Q: int, m_cap: int) -> "HorizonBounds":
        return cls(np.zeros((Q, m_cap)), np.zeros((Q, m_cap)), np.zeros(Q), np.zeros(Q))

    def as_c(self) -> abi.RlHznBnd:
        return abi.RlHznBnd(*[_ptr(getattr(self, n), np.float64, n) for n in abi.HZN_BND])


def _bnd_rows(x, y) -> tuple:
    """x, y as contiguous float64 [B, N] (one row [N] is B = 1)."""
    X = np.ascontiguousarray(x, dtype=np.float64)
    Y = np.ascontiguousarray(y, dtype=np.float64)
    if X.ndim == 1:
        X, Y = X[None], Y[None] if Y.ndim == 1 else Y
    if X.ndim != 2 or X.shape != Y.shape or X.shape[0] < 1:
        raise ValueError(f"bounds: x and y must be [B, N] with B >= 1, got {X.shape} and {Y.shape}")
    return X, Y


def _bnd_guard(veh_width, margin) -> tuple:
    try:
        w, m = float(veh_width), float(margin)
    except (TypeError, ValueError):
        raise ValueError(f"bounds: veh_width and margin must be numbers, got {veh_width!r}, {margin!r}") from None
    if not (math.isfinite(w) and math.isfinite(m)):
        raise ValueError(f"bounds: veh_width and margin must be finite, got {w}, {m}")
    return w, m


def normals_host(x, y, closed: bool) -> tuple:
    """The bounds stage's unit normals (nx, ny) [B, N] of the rows x, y [B, N] (or one row [N])
    in NumPy: normals_from_points_generic (ref:581-593) per row, +n left of travel; the kernel
    equals it bit for bit."""
    X, Y = _bnd_rows(x, y)
    n = np.stack([normals_from_points(np.stack([X[b], Y[b]], axis=1), bool(closed)) for b in range(X.shape[0])])
    n = n.reshape(X.shape[0], X.shape[1], 2)
    return np.ascontiguousarray(n[..., 0]), np.ascontiguousarray(n[..., 1])


def horizon_bounds_host(lo, hi, stamps, T, row, seg, t0, count, dt: float, m_cap: int, closed: bool) -> HorizonBounds:
    """The bounds at the horizon stage's ticks (include/rl_abi.h) in NumPy; the kernel
    equals it bit for bit.  lo, hi [R, N] are the bounds stage's rows, stamps [R, N + 1] and T [R]
    the trajectory stage's, row, seg, t0, count [Q] the horizon stage's (row None: all 0).  Tick
    m < count[q] at t0 + m * dt lies on segment i after the horizon stage's wrap and bisection,
    and gets lo = smax(lo_i, lo_j), hi = smin(hi_i, hi_j), j = (i + 1) mod N; lo0, hi0 are that
    pair of seg.  Queries with seg = -1 and the ticks from count[q] on stay NaN."""
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    if lo.ndim == 1:
        lo, hi = lo[None], hi[None]
    R, N = lo.shape
    stamps = np.ascontiguousarray(stamps, dtype=np.float64).reshape(R, N + 1)
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(R)
    seg = np.asarray(seg).reshape(-1)
    Q = seg.shape[0]
    row = np.zeros(Q, dtype=np.int64) if row is None else np.broadcast_to(np.asarray(row), (Q,))
    t0 = np.ascontiguousarray(t0, dtype=np.float64).reshape(Q)
    count = np.asarray(count).reshape(Q)
    _check_ticks(dt, m_cap)
    closed, dt, m_cap = bool(closed), float(dt), int(m_cap)
    S = N if closed else N - 1
    out = HorizonBounds.alloc(Q, m_cap)
    for a in (out.lo, out.hi, out.lo0, out.hi0):
        a[:] = np.nan

    def pair(r, i):
        j = (i + 1) % N
        a, b, c, d = lo[r, i], lo[r, j], hi[r, i], hi[r, j]
        return np.where(a < b, b, a), np.where(d < c, d, c)        # smax(lo_i, lo_j), smin(hi_i, hi_j)

    for q in range(Q):
        r, i0 = int(row[q]), int(seg[q])
        if i0 < 0 or i0 >= S or r < 0 or r >= R:
            continue
        out.lo0[q], out.hi0[q] = pair(r, i0)
        M = min(int(count[q]), m_cap)
        if M <= 0:
            continue
        with np.errstate(all="ignore"):
            tau = t0[q] + np.arange(M, dtype=np.float64) * dt
            _, w = _hzn_wrap(tau, T[r], closed)
            out.lo[q, :M], out.hi[q, :M] = pair(r, _hzn_segment(stamps[r], S, w))
    return out


def bounds(prob: Problem, x, y, veh_width: float, margin: float, device: int = 0) -> Bounds:
    """The bounds stage for B given rows x, y [B, N] (or one row [N]) on the GPU (rl_bounds): the
    rings, N and closed are prob's (its centre is not read) and go up once for all rows."""
    X, Y = _bnd_rows(x, y)
    w, m = _bnd_guard(veh_width, margin)
    B, N = X.shape
    if N != prob.N:
        raise ValueError(f"bounds: the rows have {N} samples, the problem {prob.N}")
    out = Bounds.alloc(B, N)
    p, oc = prob.as_c(), out.as_c()
    _check(_lib().rl_bounds(C.byref(p), abi.dptr(X), abi.dptr(Y), B, w, m, int(device), C.byref(oc)))
    return out


# ------------------------------------------------- recover: a path from the car's offset back to the row
@dataclass
class Recover(Retime):
    """The recover stage's answer for Q poses (rl_rcv): Retime's fields on the offset path (x, y,
    heading, kappa of the ticks leave the row; s stays the station along the row), and offset
    [Q, M_cap] (the ticks' lateral offset), clamped (nodes at which the free width cut the offset
    profile), offtrack (1: the car itself is outside lo0 .. hi0), merge_node (the first node on
    the row again, -1: not within the window), lo0, hi0 (the room at the car) [Q]; node_o, node_k
    [Q, k_cap + 1]: the nodes' offsets and the path's curvatures there."""

    offset: np.ndarray = None
    clamped: np.ndarray = None
    offtrack: np.ndarray = None
    merge_node: np.ndarray = None
    lo0: np.ndarray = None
    hi0: np.ndarray = None
    node_o: np.ndarray = None
    node_k: np.ndarray = None
    node_psi: np.ndarray = None   # [Q, k_cap + 1] the nodes' headings (host side: recover_host fills it, the library does not)

    _C = abi.RlRcv
    _COLS = abi.TRAJ_COLS + abi.RCV_COLS
    _PER = abi.HZN_LOC + abi.RCV_SCAL
    _INTS = abi.RCV_INTS
    _NODES = abi.RCV_NODES
    _HOST_NODES = ("node_psi",)

    def row(self, q: int) -> dict:
        """Retime's ticks of query q, and their offset."""
        out = super().row(q)
        out["offset"] = self.offset[q, :int(self.count[q])]
        return out


def _rcv_query(poses, v0, cfg, merge_len, dir_xy, row, seg_hint, window, dt, m_cap, k_cap) -> tuple:
    if int(k_cap) != k_cap or not 1 <= int(k_cap) <= abi.RL_RCV_MAX_NODES:
        raise ValueError(f"recover: k_cap must be 1..{abi.RL_RCV_MAX_NODES}, got {k_cap}")
    P, rw, hint, V0 = _rjn_query(poses, v0, cfg, row, seg_hint, window, dt, m_cap, k_cap)
    Q = P.shape[0]
    D = np.asarray(merge_len, dtype=np.float64)
    if D.ndim == 0:
        D = np.broadcast_to(D, (Q,))
    if D.shape != (Q,):
        raise ValueError(f"recover: merge_len must be a number or [Q={Q}] numbers, got shape {D.shape}")
    D = np.ascontiguousarray(D)
    if not np.all(np.isfinite(D)) or np.any(D <= 0.0):
        raise ValueError("recover: merge_len must be finite and > 0")
    H = None
    if dir_xy is not None:
        H = np.asarray(dir_xy, dtype=np.float64)
        if H.shape == (2,):
            H = np.broadcast_to(H, (Q, 2))
        if H.shape != (Q, 2):
            raise ValueError(f"recover: dir_xy must be [2] or [Q={Q}, 2], got shape {H.shape}")
        H = np.ascontiguousarray(H)
        if not np.all(np.isfinite(H)):
            raise ValueError("recover: dir_xy must be finite")
    return P, rw, hint, V0, D, H


def _rcv_c(P, rw, hint, V0, D, H, cfg, window, dt, m_cap, k_cap) -> abi.RlRcvQuery:
    return abi.RlRcvQuery(_rjn_c(P, rw, hint, V0, cfg, window, dt, m_cap, k_cap), _ptr(D, np.float64, "merge_len"),
                          None if H is None else _ptr(H, np.float64, "dir_xy"))


def _rcv_bounds(what: str, rows, closed: bool, lo, hi, nx, ny) -> tuple:
    """lo, hi, nx, ny as contiguous float64 [B, N] for the rows; nx, ny None: normals_host's."""
    B, N = rows[0].shape
    if nx is None or ny is None:
        nx, ny = normals_host(rows[0], rows[1], closed)
    out = []
    for name, a in zip(abi.BND_ROWS, (lo, hi, nx, ny)):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape == (N,) and B == 1:
            a = a[None]
        if a.shape != (B, N):
            raise ValueError(f"{what}: {name} must be [B={B}, N={N}], got {a.shape}")
        out.append(a)
    return tuple(out)


def _rcv_slope(dx, dy, hx, hy) -> float:
    """g0: de/ds of a car heading (hx, hy) on a segment of direction (dx, dy), capped at 45 degrees."""
    den, num = dx * hx + dy * hy, dx * hy - dy * hx
    if den > 0.0:
        return _smin(1.0, _smax(-1.0, _fdiv(num, den)))
    return -1.0 if num < 0.0 else (1.0 if num > 0.0 else 0.0)


def _rcv_quintics(z: float) -> tuple:
    """(qz, pz) at z in [0, 1]: the quintics with q(0) = 1, p'(0) = 1 and every other value, slope
    and second derivative at 0 and 1 zero; both are exactly 0.0 at z = 1."""
    z3 = (z * z) * z
    return 1.0 + z3 * (-10.0 + z * (15.0 - 6.0 * z)), z + z3 * (-6.0 + z * (8.0 - 3.0 * z))


def _rcv_geometry(o, px, py, d_row, kap_row, psi_row) -> tuple:
    """(d', kappa', psi) of the offset path through the points px, py [K + 1] with offsets o: the
    row's d_row [K], kap_row and psi_row [K + 1] where the path is on the line, the points'
    chords, Menger curvature and chord directions where it is not (§3q "geometry")."""
    K = len(o) - 1
    zero = [ok == 0.0 for ok in o]
    with np.errstate(all="ignore"):
        d = [d_row[k] if zero[k] and zero[k + 1] else
             float(np.sqrt((px[k + 1] - px[k]) * (px[k + 1] - px[k]) + (py[k + 1] - py[k]) * (py[k + 1] - py[k])))
             for k in range(K)]

        def on_line(k):
            return zero[k] and (k == 0 or zero[k - 1]) and (k == K or zero[k + 1])

        def inner(k):
            if on_line(k):
                return kap_row[k]
            ax_, ay_ = px[k] - px[k - 1], py[k] - py[k - 1]
            bx_, by_ = px[k + 1] - px[k], py[k + 1] - py[k]
            cx_, cy_ = px[k + 1] - px[k - 1], py[k + 1] - py[k - 1]
            den = (d[k - 1] * d[k]) * float(np.sqrt(cx_ * cx_ + cy_ * cy_))
            return _fdiv(2.0 * (ax_ * by_ - ay_ * bx_), den) if den > 0.0 else 0.0

        kap, psi = [0.0] * (K + 1), [0.0] * (K + 1)
        for k in range(K + 1):
            if 0 < k < K:
                kap[k] = inner(k)
            elif K < 2 or on_line(k):
                kap[k] = kap_row[k]
            else:
                kap[k] = inner(1 if k == 0 else K - 1)
            if on_line(k):
                psi[k] = psi_row[k]
            else:
                a, b = max(k - 1, 0), min(k + 1, K)
                psi[k] = math.atan2(py[b] - py[a], px[b] - px[a])
    return np.array(d, dtype=np.float64), np.array(kap, dtype=np.float64), np.array(psi, dtype=np.float64)


def recover_host(x, y, heading, kappa, v, ax, h, closed: bool, lo, hi, poses, v0, cfg: RlCfg, merge_len, dir_xy=None,
                 nx=None, ny=None, row=None, seg_hint=None, window: int = 0, dt: float = 0.05, m_cap: int = 64,
                 k_cap: int = 512, stamps=None) -> Recover:
    """The specification of the recover stage (include/rl_abi.h) in NumPy; the kernel
    equals it bit for bit (heading off the line: to the rounding of math.atan2).  The rows, poses,
    hints, stamps, v0 and cfg are retime_host's, and so are the locate and the nodes 0 .. K.  lo,
    hi [B, N] are the rows' free width (the bounds stage's) and nx, ny their unit normals (None:
    normals_host's).  From the car's offset e and slope (dir_xy: its direction of travel; None:
    along the row) a quintic offset profile runs to zero over merge_len metres along the row,
    clamped to lo .. hi at every node; the nodes moved along their normals are the path, whose
    chords, Menger curvatures and chord directions replace the row's d, kappa and heading where it
    is off the line; retime_host's ceiling, envelope and march run on that geometry, and the
    ticks m * dt before t_end follow the path.  A pose on the line heading along it gets
    retime_host's answer bit for bit."""
    closed = bool(closed)
    rows, hs, stamps, N, S, (P, rw, hint, V0, D, H) = _query_rows(
        "recover", (x, y, heading, kappa, v, ax, h), closed,
        lambda: _rcv_query(poses, v0, cfg, merge_len, dir_xy, row, seg_hint, window, dt, m_cap, k_cap), stamps)
    LO, HI, NX, NY = _rcv_bounds("recover", rows, closed, lo, hi, nx, ny)
    Q, dt, m_cap, W, k_cap = P.shape[0], float(dt), int(m_cap), int(window), int(k_cap)
    consts = _rjn_consts(cfg)
    out = Recover.alloc(Q, m_cap, dt, k_cap)
    out.seg[:] = -1
    out.end_node[:] = -1
    tau_all = np.arange(m_cap, dtype=np.float64) * dt
    for q in range(Q):
        if S < 1:
            continue
        row6 = [a[rw[q]] for a in rows]
        X, Y = row6[:2]
        blo, bhi, bnx, bny = (a[rw[q]] for a in (LO, HI, NX, NY))
        t, hb = stamps[rw[q]], float(hs[rw[q]])
        T = t[S]
        px, py = P[q, 0], P[q, 1]
        loc = _hzn_locate(X, Y, t, hb, px, py, int(hint[q]), W, closed)
        if loc is None:
            continue
        i0, u, t0 = int(loc[0]), float(loc[1]), loc[4]
        K = min(k_cap, N if closed else N - 1 - i0)
        if K < 1:
            continue
        out.seg[q], out.u[q], out.dist2[q], out.e[q], out.t0[q], out.s0[q] = loc
        e, Dq, j0 = float(loc[3]), float(D[q]), (i0 + 1) % N
        nodes = n, idx, kap, r, d0 = _march_nodes(row6, i0, u, hb, K)
        with np.errstate(all="ignore"):
            dx, dy, wx, wy = float(X[j0] - X[i0]), float(Y[j0] - Y[i0]), float(px - X[i0]), float(py - Y[i0])
            g0 = 0.0 if H is None else _rcv_slope(dx, dy, float(H[q, 0]), float(H[q, 1]))
            gD = g0 * Dq
            o, ncl, mg = [e], 0, -1                                    # offsets and clamp
            for k in range(1, K + 1):
                z = _smin(1.0, _fdiv(float(d0) + float(k - 1) * hb, Dq))
                qz, pz = _rcv_quintics(z)
                raw = e * qz + gD * pz
                ok = _smin(float(bhi[idx[k]]), _smax(float(blo[idx[k]]), raw))
                o.append(ok)
                ncl += ok != raw
                if mg < 0 and z >= 1.0:
                    mg = k
            lo0, hi0 = _smax(float(blo[i0]), float(blo[j0])), _smin(float(bhi[i0]), float(bhi[j0]))
            values = nxv, nyv, npsi, ns = _node_values(row6, nodes, i0, u, hb, out.s0[q])
            o = np.array(o, dtype=np.float64)
            ppx, ppy = X[idx] + o * bnx[idx], Y[idx] + o * bny[idx]    # points
            ppx[0], ppy[0] = nxv[0] + (wx - u * dx), nyv[0] + (wy - u * dy)
            d_row = np.concatenate(([d0], np.full(K - 1, hb)))
            dp, kp, psi = _rcv_geometry(o.tolist(), ppx.tolist(), ppy.tolist(), d_row.tolist(), kap.tolist(), npsi.tolist())
        w, tt, b, c, over, ve, bind = _retime_pass(consts, cfg, float(V0[q]), kp, r, dp.tolist())
        out.node_v[q, :K + 1], out.node_t[q, :K + 1], out.node_b[q, :K + 1], out.node_c[q, :K + 1] = w, tt, b, c
        out.node_o[q, :K + 1], out.node_k[q, :K + 1], out.node_psi[q, :K + 1] = o, kp, psi
        tte = tt[K]
        out.end_node[q], out.overspeed[q], out.feasible[q] = K, over, 1 if float(V0[q]) <= b[0] else 0
        out.bind_node[q], out.t_end[q], out.v_excess[q] = bind, tte, ve
        out.clamped[q], out.merge_node[q], out.offtrack[q] = ncl, mg, 0 if (lo0 <= e and e <= hi0) else 1
        out.lo0[q], out.hi0[q] = lo0, hi0
        nk = i0 + K
        c0 = nk // N
        with np.errstate(all="ignore"):
            out.t_loss[q] = tte - ((np.float64(c0) * T + t[nk - c0 * N]) - t0)
            M1 = int(np.count_nonzero(tau_all < tte))           # (monotone in m: the kernel bisects)
            out.count[q] = M1
            if M1 > 0:
                a, um = _node_ticks(out, q, M1, tau_all[:M1], tt, w, K, (ppx, ppy, psi, ns), kp, dp)
                out.offset[q, :M1] = o[a] + um * (o[a + 1] - o[a])
    return out


def recover(x, y, heading, kappa, v, ax, h, closed: bool, lo, hi, poses, v0, cfg: RlCfg, merge_len, dir_xy=None,
            nx=None, ny=None, row=None, seg_hint=None, window: int = 0, dt: float = 0.05, m_cap: int = 64,
            k_cap: int = 512, device: int = 0) -> Recover:
    """recover_host on the GPU (rl_recover): the trajectory kernel stamps the B given rows, then
    the recover kernel answers the Q poses on them and their bounds; row[q] counts the given rows."""
    rows, hs, (P, rw, hint, V0, D, H), B, N = _open_query(
        "recover", (x, y, heading, kappa, v, ax, h),
        lambda: _rcv_query(poses, v0, cfg, merge_len, dir_xy, row, seg_hint, window, dt, m_cap, k_cap))
    bnd = _rcv_bounds("recover", rows, bool(closed), lo, hi, nx, ny)
    out = Recover.alloc(P.shape[0], int(m_cap), dt, int(k_cap))
    qc, oc = _rcv_c(P, rw, hint, V0, D, H, cfg, window, dt, m_cap, k_cap), out.as_c()
    _check(_lib().rl_recover(*[_ptr(a, np.float64, "row") for a in rows], _ptr(hs, np.float64, "h"),
                             *[_ptr(a, np.float64, "bounds") for a in bnd], N, B, 1 if closed else 0, C.byref(qc),
                             int(device), C.byref(oc)))
    return out


# ------------------------------------------------- fan: several merge lengths per pose, the best one served
@dataclass
class RecoverFan(Recover):
    """The fan stage's answer for Q poses and C merge lengths each (rl_fan): Recover's fields hold
    the winner's values; best [Q] is the winner's candidate (-1: an empty query); cand_class,
    cand_feasible, cand_clamped, cand_merge_node, cand_overspeed, cand_bind_node, cand_t_end,
    cand_t_loss, cand_v_excess [Q, C] are every candidate's per-query values."""

    best: np.ndarray = None
    cand_class: np.ndarray = None
    cand_feasible: np.ndarray = None
    cand_clamped: np.ndarray = None
    cand_merge_node: np.ndarray = None
    cand_overspeed: np.ndarray = None
    cand_bind_node: np.ndarray = None
    cand_t_end: np.ndarray = None
    cand_t_loss: np.ndarray = None
    cand_v_excess: np.ndarray = None

    _C = abi.RlFan
    _INTS = abi.RCV_INTS + ("best",)
    _TAB_INTS = abi.FAN_TAB_INTS
    _TAB_PER = abi.FAN_TAB_SCAL


def fan_order(feasible, clamped, merge_node, t_end) -> tuple:
    """The fan stage's order alone.  For tables [Q, C] (or [C]) of the candidates' feasible,
    clamped, merge_node and t_end: cls, the classes (0: feasible, not clamped and merged; 1:
    feasible and merged; 2: feasible; 3: otherwise), and best [Q] (or a number), the first
    candidate ascending in (cls, isnan(t_end), t_end, c), with plain < on doubles."""
    fe, cl, mn = (np.asarray(a) for a in (feasible, clamped, merge_node))
    te = np.asarray(t_end, dtype=np.float64)
    one = te.ndim == 1
    fe, cl, mn, te = (np.atleast_2d(a) for a in (fe, cl, mn, te))
    if not (fe.shape == cl.shape == mn.shape == te.shape) or te.shape[1] < 1:
        raise ValueError(f"fan_order: the four tables must have one shape [Q, C >= 1], got {fe.shape}, {cl.shape}, {mn.shape}, {te.shape}")
    cls = np.where(fe == 0, 3, np.where(mn < 0, 2, np.where(cl != 0, 1, 0))).astype(np.int32)
    best = np.zeros(te.shape[0], dtype=np.int32)
    for q in range(te.shape[0]):
        b = 0
        for c in range(1, te.shape[1]):
            ka = (int(cls[q, c]), bool(np.isnan(te[q, c])))
            kb = (int(cls[q, b]), bool(np.isnan(te[q, b])))
            if ka < kb or (ka == kb and te[q, c] < te[q, b]):
                b = c
        best[q] = b
    return (cls[0], int(best[0])) if one else (cls, best)


def _fan_query(poses, v0, cfg, merge_lens, dir_xy, row, seg_hint, window, dt, m_cap, k_cap) -> tuple:
    """_rcv_query's arrays with D [Q, C] from merge_lens [C] or [Q, C]."""
    Q = np.asarray(poses, dtype=np.float64).reshape(-1, 2).shape[0] if np.size(poses) else 0
    D = np.asarray(merge_lens, dtype=np.float64)
    if D.ndim == 1:
        D = np.broadcast_to(D, (Q, D.shape[0]))
    if D.ndim != 2 or D.shape[0] != Q or not 1 <= D.shape[1] <= abi.RL_FAN_MAX_CAND:
        raise ValueError(f"recover_fan: merge_lens must be [C] or [Q={Q}, C] with C in 1..{abi.RL_FAN_MAX_CAND}, got shape {D.shape}")
    if Q * D.shape[1] > abi.RL_HZN_MAX_QUERIES:
        raise ValueError(f"recover_fan: Q*C must be <= {abi.RL_HZN_MAX_QUERIES}, got {Q * D.shape[1]}")
    D = np.ascontiguousarray(D)
    if not np.all(np.isfinite(D)) or np.any(D <= 0.0):
        raise ValueError("recover_fan: merge_lens must be finite and > 0")
    P, rw, hint, V0, _, H = _rcv_query(poses, v0, cfg, D[:, 0], dir_xy, row, seg_hint, window, dt, m_cap, k_cap)
    return P, rw, hint, V0, D, H


def _fan_c(P, rw, hint, V0, D, H, cfg, window, dt, m_cap, k_cap) -> abi.RlFanQuery:
    return abi.RlFanQuery(_rcv_c(P, rw, hint, V0, D, H, cfg, window, dt, m_cap, k_cap), D.shape[1], 0)


def recover_fan_host(x, y, heading, kappa, v, ax, h, closed: bool, lo, hi, poses, v0, cfg: RlCfg, merge_lens, dir_xy=None,
                     nx=None, ny=None, row=None, seg_hint=None, window: int = 0, dt: float = 0.05, m_cap: int = 64,
                     k_cap: int = 512, stamps=None) -> RecoverFan:
    """The specification of the fan stage (include/rl_abi.h) in NumPy: recover_host
    once per candidate length (merge_lens [C] or [Q, C]), fan_order on the candidates' feasible,
    clamped, merge_node and t_end, and every field of the winner.  An empty query (end_node = -1)
    has best = -1, seg and count = 0 as recover_host gives them and nothing else specified."""
    P, rw, hint, V0, D, H = _fan_query(poses, v0, cfg, merge_lens, dir_xy, row, seg_hint, window, dt, m_cap, k_cap)
    Q, Cn = D.shape
    cands = [recover_host(x, y, heading, kappa, v, ax, h, closed, lo, hi, P, V0, cfg, D[:, c], H, nx, ny, rw, hint, window,
                          dt, m_cap, k_cap, stamps) for c in range(Cn)]
    out = RecoverFan.alloc(Q, int(m_cap), dt, int(k_cap), Cn)
    table = {"cand_feasible": "feasible", "cand_clamped": "clamped", "cand_merge_node": "merge_node",
             "cand_overspeed": "overspeed", "cand_bind_node": "bind_node", "cand_t_end": "t_end", "cand_t_loss": "t_loss",
             "cand_v_excess": "v_excess"}
    for name, src in table.items():
        getattr(out, name)[:] = np.stack([getattr(r, src) for r in cands], axis=1)
    out.cand_class[:], out.best[:] = fan_order(out.cand_feasible, out.cand_clamped, out.cand_merge_node, out.cand_t_end)
    fields = [f for f in Recover.__dataclass_fields__ if isinstance(getattr(out, f), np.ndarray)]
    for q in range(Q):
        if cands[0].end_node[q] < 0:                   # (every candidate shares the locate)
            out.best[q] = -1
        win = cands[max(int(out.best[q]), 0)]
        for f in fields:
            getattr(out, f)[q] = getattr(win, f)[q]
    return out


def recover_fan(x, y, heading, kappa, v, ax, h, closed: bool, lo, hi, poses, v0, cfg: RlCfg, merge_lens, dir_xy=None,
                nx=None, ny=None, row=None, seg_hint=None, window: int = 0, dt: float = 0.05, m_cap: int = 64,
                k_cap: int = 512, device: int = 0) -> RecoverFan:
    """recover_fan_host on the GPU (rl_recover_fan): the trajectory kernel stamps the B given
    rows, then the fan stage's kernels answer the Q poses with C merge lengths each."""
    rows, hs, (P, rw, hint, V0, D, H), B, N = _open_query(
        "recover_fan", (x, y, heading, kappa, v, ax, h),
        lambda: _fan_query(poses, v0, cfg, merge_lens, dir_xy, row, seg_hint, window, dt, m_cap, k_cap))
    bnd = _rcv_bounds("recover_fan", rows, bool(closed), lo, hi, nx, ny)
    out = RecoverFan.alloc(P.shape[0], int(m_cap), dt, int(k_cap), D.shape[1])
    qc, oc = _fan_c(P, rw, hint, V0, D, H, cfg, window, dt, m_cap, k_cap), out.as_c()
    _check(_lib().rl_recover_fan(*[_ptr(a, np.float64, "row") for a in rows], _ptr(hs, np.float64, "h"),
                                 *[_ptr(a, np.float64, "bounds") for a in bnd], N, B, 1 if closed else 0, C.byref(qc),
                                 int(device), C.byref(oc)))
    return out


# ------------------------------------------------- rollouts: sampled trajectories scored against the plan
@dataclass
class Rollouts:
    """The scores of Q rollouts of T poses (rl_rll).  Per pose [Q, T]: seg (-1 from the end of the
    chain on), u, e, dist2 as the horizon stage's location, s (arc length, counted on across the
    start line), margin (the room left to the nearer bound, negative outside) and vref (the row's
    speed there); they are None when the fetch left them on the device.  Per rollout [Q]: count
    (poses located before the chain ended), valid (count == T), first_out (the first pose with
    margin < 0, T: none), progress, e_max, margin_min and cost.  order [G, k]: the k best rollouts
    of each group, ascending in (isnan(cost), cost, index)."""

    seg: Optional[np.ndarray]
    u: Optional[np.ndarray]
    e: Optional[np.ndarray]
    dist2: Optional[np.ndarray]
    s: Optional[np.ndarray]
    margin: Optional[np.ndarray]
    vref: Optional[np.ndarray]
    count: np.ndarray
    valid: np.ndarray
    first_out: np.ndarray
    progress: np.ndarray
    e_max: np.ndarray
    margin_min: np.ndarray
    cost: np.ndarray
    order: np.ndarray

    _C, _NODES = abi.RlRll, ()          # (Plan._stage_fetch)

    @classmethod
    def alloc(cls, Q: int, T: int, G: int, k: int, poses: bool = True) -> "Rollouts":
        per = {n: np.zeros((Q, T)) if poses else None for n in abi.RLL_POSE}
        return cls(seg=np.zeros((Q, T), dtype=np.int32) if poses else None, **per,
                   **{n: np.zeros(Q, dtype=np.int32) for n in abi.RLL_INTS}, **{n: np.zeros(Q) for n in abi.RLL_SCAL},
                   order=np.zeros((G, k), dtype=np.int32))

    def as_c(self) -> abi.RlRll:
        t = abi.RlRll()
        for n in ("seg",) + abi.RLL_INTS + ("order",):
            if getattr(self, n) is not None:
                setattr(t, n, _ptr(getattr(self, n), np.int32, n))
        for n in abi.RLL_POSE + abi.RLL_SCAL:
            if getattr(self, n) is not None:
                setattr(t, n, _ptr(getattr(self, n), np.float64, n))
        return t


ROLLOUT_WEIGHTS = (1.0, 1.0, 1.0, 1.0)      # w_e, w_out, w_v, w_prog


def _rll_query(xy, v, row, seg_hint, window0, window, weights, hard_bounds, group_size, k) -> tuple:
    """The query as arrays and numbers: xy [Q, T, 2] float64, v [Q, T] float64 or None, row and
    seg_hint [Q] int32 or None, the windows, the four weights, hard_bounds, the group size and k."""
    P = np.ascontiguousarray(xy, dtype=np.float64)
    if P.ndim == 2 and P.shape[1] == 2:
        P = P[None]
    if P.ndim != 3 or P.shape[2] != 2 or not 1 <= P.shape[0] <= abi.RL_RLL_MAX_ROLLOUTS or \
            not 1 <= P.shape[1] <= abi.RL_RLL_MAX_STEPS or P.shape[0] * P.shape[1] > abi.RL_RLL_MAX_POSES:
        raise ValueError(f"rollouts: xy must be [Q, T, 2] with 1 <= Q <= {abi.RL_RLL_MAX_ROLLOUTS}, 1 <= T <= "
                         f"{abi.RL_RLL_MAX_STEPS} and Q*T <= {abi.RL_RLL_MAX_POSES}, got shape {P.shape}")
    Q, T = P.shape[:2]
    V = None
    if v is not None:
        V = np.ascontiguousarray(v, dtype=np.float64)
        if V.shape == (T,) and Q == 1:
            V = V[None]
        if V.shape != (Q, T):
            raise ValueError(f"rollouts: v must be [Q={Q}, T={T}], got shape {V.shape}")

    def ints(a, name):
        if a is None:
            return None
        a = np.asarray(a)
        if a.ndim == 0:
            a = np.broadcast_to(a, (Q,))
        if a.shape != (Q,) or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"rollouts: {name} must be an integer or [Q={Q}] integers, got {a.dtype} {a.shape}")
        return np.ascontiguousarray(a, dtype=np.int32)

    for name, w in (("window0", window0), ("window", window)):
        if int(w) != w or w < 0 or w >= 2 ** 31:
            raise ValueError(f"rollouts: {name} must be an integer >= 0, got {w}")
    wts = tuple(float(w) for w in weights)
    if len(wts) != 4 or not all(np.isfinite(w) and w >= 0.0 for w in wts):
        raise ValueError(f"rollouts: weights must be four finite numbers >= 0 (w_e, w_out, w_v, w_prog), got {weights}")
    gs = Q if group_size in (None, 0) else int(group_size)
    if gs < 1 or Q % gs != 0:
        raise ValueError(f"rollouts: Q={Q} is not a multiple of group_size={group_size}")
    if not 1 <= int(k) <= min(gs, abi.RL_SELECT_MAX_K):
        raise ValueError(f"rollouts: need 1 <= k <= min(group_size={gs}, {abi.RL_SELECT_MAX_K}), got {k}")
    hint = ints(seg_hint, "seg_hint")
    if hint is not None and np.any(hint < -1):
        raise ValueError("rollouts: seg_hint < -1")
    return P, V, ints(row, "row"), hint, int(window0), int(window), wts, bool(hard_bounds), gs, int(k)


def _rll_c(qy) -> abi.RlRllQuery:
    P, V, rw, hint, W0, W, wts, hard, gs, k = qy
    return abi.RlRllQuery(_ptr(P, np.float64, "xy"), None if V is None else _ptr(V, np.float64, "v"),
                          None if rw is None else _ptr(rw, np.int32, "row"),
                          None if hint is None else _ptr(hint, np.int32, "seg_hint"), P.shape[0], P.shape[1], W0, W,
                          *wts, 1 if hard else 0, gs, k, 0)


def _rll_bounds(rows, lo, hi) -> tuple:
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    if lo.ndim == 1:
        lo, hi = lo[None], hi[None]
    if lo.shape != rows[0].shape or hi.shape != rows[0].shape:
        raise ValueError(f"rollouts: lo and hi must have the rows' shape {rows[0].shape}, got {lo.shape} and {hi.shape}")
    return lo, hi


def rank_order(cost, k: int, group_size: int) -> np.ndarray:
    """index [G, k]: rank_scores' order in NumPy: the global indices of the k least of each group of
    group_size, ascending in (isnan(cost), cost, index); -0.0 and 0.0 tie."""
    cost = np.asarray(cost, dtype=np.float64).ravel()
    G = cost.shape[0] // group_size
    out = np.zeros((G, k), dtype=np.int32)
    for g in range(G):
        c = cost[g * group_size:(g + 1) * group_size]
        nan = np.isnan(c)
        out[g] = g * group_size + np.lexsort((np.arange(group_size), np.where(nan, 0.0, c), nan))[:k]
    return out


def rollouts_host(x, y, heading, kappa, v, ax, h, closed: bool, lo, hi, xy, speeds=None, row=None, seg_hint=None,
                  window0: int = 0, window: int = 8, weights=ROLLOUT_WEIGHTS, hard_bounds: bool = False,
                  group_size: Optional[int] = None, k: int = 1) -> Rollouts:
    """The specification of the rollout stage (include/rl_abi.h) in NumPy; the kernel
    equals it bit for bit.  Rows [B, N] (or one row [N]) with steps h as for trajectory_host, and
    their bounds rows lo, hi [B, N] (the bounds stage's).  Rollout q, poses xy[q] [T, 2] with
    optional speeds speeds[q] [T], lies on row[q] (None: row 0).  Pose 0 is located as the horizon
    stage locates a pose with hint seg_hint[q] (None or -1: every segment; a hint past an open row
    has no candidate) and window0; pose t >= 1 with the segment found for pose t - 1 as its hint and
    `window`.  The first pose without a winner ends the chain: count = t, NaN and seg = -1 from
    there on, valid = 0, progress and cost NaN.  c counts the crossings of the start line on a
    closed row (a jump of more than half the row backward is a crossing forward, and the other way
    round), s = ((c*S + seg) + u)*h, margin = smin(hi_t - e, e - lo_t) with horizon_bounds_host's
    pair of the segment, vref the row's speed at the foot.  The sums E, O, V are added serially in
    ascending t from 0.0; cost = ((w_e*E + w_out*O) + w_v*V) - w_prog*progress, +inf with
    hard_bounds when a pose lies outside.  order is rank_order's."""
    closed = bool(closed)
    rows, hs, qy, B, N = _open_query("rollouts", (x, y, heading, kappa, v, ax, h),
                                     lambda: _rll_query(xy, speeds, row, seg_hint, window0, window, weights, hard_bounds,
                                                        group_size, k))
    lo, hi = _rll_bounds(rows, lo, hi)
    P, VQ, rw, hint, W0, W, (w_e, w_out, w_v, w_prog), hard, gs, k = qy
    Q, T = P.shape[:2]
    S = N if closed else N - 1
    rw = np.zeros(Q, dtype=np.int32) if rw is None else rw
    hint = np.full(Q, -1, dtype=np.int32) if hint is None else hint
    if np.any(rw < 0) or np.any(rw >= B):
        raise ValueError(f"rollouts: row outside [0, {B})")
    out = Rollouts.alloc(Q, T, Q // gs, k)
    out.seg[:] = -1
    for n in abi.RLL_POSE:
        getattr(out, n)[:] = np.nan
    nostamps = np.zeros(N + 1)                                  # (the chain needs no time on the row)
    f64 = np.float64
    with np.errstate(all="ignore"):
        for q in range(Q):
            r = int(rw[q])
            X, Y, Vr, hb = rows[0][r], rows[1][r], rows[4][r], hs[r]
            g, c, cnt = int(hint[q]), 0, T
            E = O = V = e_max = f64(0.0)
            m_min, first_out = f64(np.inf), T
            for t in range(T):
                loc = _hzn_locate(X, Y, nostamps, hb, P[q, t, 0], P[q, t, 1], g, W0 if t == 0 else W, closed) if S >= 1 else None
                if loc is None:
                    cnt = t
                    break
                i, u, D, e = loc[:4]
                if closed and t > 0:
                    d = i - g
                    c += 1 if 2 * d < -S else (-1 if 2 * d > S else 0)
                g = i
                j = (i + 1) % N
                a, b, lo2, hi2 = lo[r, i], lo[r, j], hi[r, i], hi[r, j]
                lo_t, hi_t = (b if a < b else a), (hi2 if hi2 < lo2 else lo2)       # smax(lo_i, lo_j), smin(hi_i, hi_j)
                m1, m2 = hi_t - e, e - lo_t
                m = m2 if m2 < m1 else m1                                             # smin(hi_t - e, e - lo_t)
                vref = Vr[i] + u * (Vr[j] - Vr[i])
                out.seg[q, t], out.u[q, t], out.e[q, t], out.dist2[q, t] = i, u, e, D
                out.s[q, t] = ((f64(c) * f64(S) + f64(i)) + u) * hb
                out.margin[q, t], out.vref[q, t] = m, vref
                E = E + e * e
                O = O + (m * m if m < 0.0 else f64(0.0))
                if VQ is not None:
                    dv = VQ[q, t] - vref
                    V = V + dv * dv
                ae = np.abs(e)
                e_max = ae if e_max < ae else e_max
                m_min = m if m < m_min else m_min
                if m < 0.0 and first_out == T:
                    first_out = t
            out.count[q], out.valid[q], out.first_out[q] = cnt, 1 if cnt == T else 0, first_out
            out.e_max[q], out.margin_min[q] = e_max, m_min
            out.progress[q] = out.cost[q] = np.nan
            if cnt == T:
                prog = out.s[q, T - 1] - out.s[q, 0]
                out.progress[q] = prog
                out.cost[q] = ((w_e * E + w_out * O) + w_v * V) - w_prog * prog
                if hard and first_out < T:
                    out.cost[q] = np.inf
    out.order[:] = rank_order(out.cost, k, gs)
    return out


def rollouts(x, y, heading, kappa, v, ax, h, closed: bool, lo, hi, xy, speeds=None, row=None, seg_hint=None,
             window0: int = 0, window: int = 8, weights=ROLLOUT_WEIGHTS, hard_bounds: bool = False,
             group_size: Optional[int] = None, k: int = 1, poses: bool = True, device: int = 0) -> Rollouts:
    """rollouts_host on the GPU (rl_rollouts): the rollout kernel on the B given rows and their bounds
    rows, then the rank kernel on the costs; row[q] counts the given rows.  poses=False leaves the
    per-pose arrays on the device."""
    rows, hs, qy, B, N = _open_query("rollouts", (x, y, heading, kappa, v, ax, h),
                                     lambda: _rll_query(xy, speeds, row, seg_hint, window0, window, weights, hard_bounds,
                                                        group_size, k))
    lo, hi = _rll_bounds(rows, lo, hi)
    Q, T = qy[0].shape[:2]
    out = Rollouts.alloc(Q, T, Q // qy[8], qy[9], poses)
    qc, oc = _rll_c(qy), out.as_c()
    _check(_lib().rl_rollouts(*[_ptr(a, np.float64, "row") for a in rows], _ptr(hs, np.float64, "h"),
                              _ptr(lo, np.float64, "lo"), _ptr(hi, np.float64, "hi"), N, B, 1 if closed else 0,
                              C.byref(qc), int(device), C.byref(oc)))
    return out


def path_lengths(x, y, closed: bool, device: int = 0) -> np.ndarray:
    """L [B]: the debug dump's path_length (ref:1443-1448) of B paths given as rows x [B, N],
    y [B, N], summed on the GPU in the reference's order (rl_path_lengths): L[b] equals
    path_length(column_stack(x[b], y[b]), closed) bit for bit."""
    X = np.ascontiguousarray(x, dtype=np.float64)
    Y = np.ascontiguousarray(y, dtype=np.float64)
    if X.ndim == 1:
        X, Y = X[None], Y[None]
    if X.ndim != 2 or X.shape != Y.shape or X.shape[0] < 1:
        raise ValueError(f"path_lengths: x and y must be [B, N] arrays of one shape, got {X.shape} and {Y.shape}")
    B, N = X.shape
    L = np.zeros(B)
    if N == 0:                              # (no row to point at)
        X = Y = np.zeros((B, 1))
    _check(_lib().rl_path_lengths(abi.dptr(X), abi.dptr(Y), N, B, 1 if closed else 0, int(device), abi.dptr(L)))
    return L


def rank_scores(scores, k: int, group_size: Optional[int] = None, device: int = 0) -> np.ndarray:
    """index [G, k] of the k best of each group of caller-supplied scores, in the order of
    rl_plan_select: ascending in (isnan, score, index) (rl_rank_scores, the same kernel)."""
    sc = np.ascontiguousarray(scores, dtype=np.float64).ravel()
    B = int(sc.size)
    if group_size in (None, 0):
        group_size = B
    if B < 1 or group_size < 1 or B % group_size != 0:
        raise ValueError(f"group_size: B={B} is not a multiple of {group_size}")
    if not 1 <= k <= min(group_size, abi.RL_SELECT_MAX_K):
        raise ValueError(f"k: need 1 <= k <= min(group_size={group_size}, {abi.RL_SELECT_MAX_K}), got {k}")
    index = np.zeros((B // group_size, k), dtype=np.int32)
    _check(_lib().rl_rank_scores(abi.dptr(sc), B, int(group_size), int(k), int(device), abi.iptr(index)))
    return index


_STAGE_RESULTS = {"horizon": Horizon, "rejoin": Rejoin, "stop": Stop, "retime": Retime, "recover": Recover,
                  "recover_fan": RecoverFan, "trajectory": Trajectory, "bounds": Bounds, "horizon_bounds": HorizonBounds,
                  "rollouts": Rollouts}


class Plan:
    """Device-resident batch (rl_plan_*): inputs uploaded once, run() enqueues
    the optimisation on a HIP stream, fetch() copies results to the host."""

    def __init__(self, prob: Problem, cfgs, seeds=None, B: Optional[int] = None, modes: int = abi.RL_MODE_MINCURV,
                 device: int = 0):
        cfg_arr, ncfg = abi.cfg_array(cfgs)
        if B is None:
            B = ncfg if ncfg > 1 else (len(seeds) if seeds is not None else 1)
        _check_batch(B, ncfg, seeds)
        self.B, self.N, self.modes = B, prob.N, modes
        self.max_outer = int(cfg_arr[0].max_outer_iters)
        self._keep = (prob, cfg_arr)
        seeds_a = abi.seed_array(seeds)
        h = C.c_void_p()
        p = prob.as_c()
        _check(_lib().rl_plan_create(C.byref(h), device, C.byref(p), cfg_arr, ncfg, abi.u64ptr(seeds_a), B, modes))
        self._h = h

    def run(self, stream_ptr: int = 0) -> None:
        _check(_lib().rl_plan_run(self._h, C.c_void_p(stream_ptr) if stream_ptr else None))

    @staticmethod
    def run_group(plans: Sequence["Plan"], stream_ptr: int = 0) -> None:
        """rl_plan_run_group: run the plans (one device) in as few kernel launches as their
        shapes allow -- a sweep of small plans as a few large grids -- with results equal to
        each plan's own run().  `stream_ptr` (0: the first plan's stream) waits for all."""
        if not plans or any(getattr(pl, "_h", None) is None for pl in plans):
            raise ValueError("run_group: no plans, or a closed plan")
        hs = (C.c_void_p * len(plans))(*[pl._h.value for pl in plans])
        _check(_lib().rl_plan_run_group(hs, len(plans), C.c_void_p(stream_ptr) if stream_ptr else None))

    def set_shape_batch(self, shape_B: int) -> None:
        """Choose the kernel shape for a batch of shape_B instances (0 = this plan's B):
        rl_plan_set_shape_batch.  Concurrent plans on one device pass the total in flight."""
        _check(_lib().rl_plan_set_shape_batch(self._h, int(shape_B)))

    def shape(self, mode: int) -> tuple:
        """(K, T) of the kernel rl_plan_run launches for `mode` (K = 0: streaming kernel)."""
        k, t = C.c_int32(), C.c_int32()
        _check(_lib().rl_plan_shape(self._h, int(mode), C.byref(k), C.byref(t)))
        return k.value, t.value

    def kernel_ms(self, idx: int) -> float:
        ms = C.c_float()
        _check(_lib().rl_plan_kernel_ms(self._h, idx, C.byref(ms)))
        return float(ms.value)

    def fetch(self):
        out_mc = Outputs.alloc(self.B, self.N, self.max_outer, False) if self.modes & abi.RL_MODE_MINCURV else None
        out_mt = Outputs.alloc(self.B, self.N, self.max_outer, True) if self.modes & abi.RL_MODE_MINTIME else None
        c_mc = out_mc.as_c() if out_mc else None
        c_mt = out_mt.as_c() if out_mt else None
        _check(_lib().rl_plan_fetch(self._h, C.byref(c_mc) if c_mc else None, C.byref(c_mt) if c_mt else None))
        return out_mc, out_mt

    def lap(self, stream_ptr: int = 0) -> None:
        """Enqueue the lap stage after the last run() (rl_plan_lap): every min-curvature
        raceline's own path length, then heading, curvature and the velocity profile with
        h = path length / N -- the debug dump's "min-curv lap" for the whole batch."""
        _check(_lib().rl_plan_lap(self._h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def fetch_lap(self):
        """Download the last lap(): (Outputs, path_len [B]).  The Outputs hold heading, kappa,
        v, ax, lap and vpass_sweeps [B, 1] as lap_eval returns them; x, y and the alphas are
        not part of the stage and stay zero."""
        out = Outputs.alloc(self.B, self.N, 0, True)
        path_len = np.zeros(self.B)
        o = out.as_c()
        _check(_lib().rl_plan_fetch_lap(self._h, C.byref(o), abi.dptr(path_len)))
        return out, path_len

    def select(self, mode="mintime", k: int = 1, group_size: Optional[int] = None, stream_ptr: int = 0,
               score="default") -> None:
        """Enqueue score -> rank -> gather after the last run() (rl_plan_select): the k best
        instances of each group of group_size (None: all B) in `mode`.  score="lap" ranks
        min-curvature racelines by the lap stage's lap (rl_plan_select_scored; runs lap()
        first unless one is valid since the last run)."""
        m, gs = _check_select(self.B, mode, k, group_size)
        by_lap = _check_score(score, m)
        s = abi.RlSelect(m, k, gs, 0)
        st = C.c_void_p(stream_ptr) if stream_ptr else None
        self._shapes["selected"] = None
        if _SCORES[score] == abi.RL_SCORE_DEFAULT:
            _check(_lib().rl_plan_select(self._h, C.byref(s), st))
        else:
            _check(_lib().rl_plan_select_scored(self._h, C.byref(s), _SCORES[score], st))
        self._shapes["selected"] = (m, k, gs, by_lap)

    def fetch_selected(self) -> Selected:
        """Download the last select(): indices, scores and the winners' rows (rl_plan_fetch_selected)."""
        if self._shapes.get("selected") is None:
            raise ValueError("fetch_selected: no select() on this plan")
        m, k, gs, by_lap = self._shapes["selected"]
        sel = _selected_alloc(self.B, self.N, self.max_outer, m, k, gs, by_lap)
        o = sel.out.as_c()
        _check(_lib().rl_plan_fetch_selected(self._h, abi.iptr(sel.index), abi.dptr(sel.score),
                                             abi.dptr(sel.scores), C.byref(o)))
        return sel

    def trajectory(self, mode="mintime", dt: float = 0.05, m_cap: int = 1024, rows="all", stream_ptr: int = 0) -> None:
        """Enqueue the trajectory stage after the last run() (rl_plan_trajectory): the state at
        the ticks m * dt, at most m_cap per row, of every instance (rows="all") or of the
        winners of the last select() of the same mode (rows="selected").  Min-curvature rows
        take heading, curvature, v and ax from the lap stage (run first unless one is valid)."""
        if mode not in _MODES:
            raise ValueError(f"mode must be 'mincurv' or 'mintime', got {mode!r}")
        if rows not in _TRAJ_ROWS:
            raise ValueError(f"rows must be 'all' or 'selected', got {rows!r}")
        sel = self._shapes.get("selected")  # (rows="selected" without one: the library refuses the call)
        R = self.B if rows == "all" or sel is None else (self.B // sel[2]) * sel[1]
        self._stage_enqueue("trajectory", (R, self.N, int(m_cap), float(dt)), stream_ptr, _MODES[mode], _TRAJ_ROWS[rows],
                            float(dt), int(m_cap))

    def fetch_trajectory(self) -> Trajectory:
        """Download the last trajectory() (rl_plan_fetch_trajectory)."""
        return self._stage_fetch("trajectory")

    # Every stage but the lap stage and the selection: `kind` names the C entry points
    # rl_plan_<kind> and rl_plan_fetch_<kind>, the public methods <kind>() and fetch_<kind>() and, in
    # _STAGE_RESULTS, the result class.  _shapes[kind], the shape of the last enqueued stage of the
    # kind (the arguments of the class's alloc), is what its fetch allocates; None: no stage, or one
    # that failed.  (_shapes["selected"] is the last select()'s mode, k, group size and score.)
    @property
    def _shapes(self) -> dict:
        return self.__dict__.setdefault("_stage_shapes", {})

    def _stage_enqueue(self, kind: str, shape: tuple, stream_ptr: int, *args) -> None:
        self._shapes[kind] = None
        _check(getattr(_lib(), "rl_plan_" + kind)(self._h, *args, C.c_void_p(stream_ptr) if stream_ptr else None))
        self._shapes[kind] = shape

    def _stage_fetch(self, kind: str, nodes: bool = True, *more):
        cls, fetch = _STAGE_RESULTS[kind], getattr(_lib(), "rl_plan_fetch_" + kind)
        shape = self._shapes.get(kind)
        if shape is None:
            t = cls._C()                    # (the library's own answer: no stage on this plan)
            _check(fetch(self._h, C.byref(t)))
            raise ValueError(f"fetch_{kind}: no {kind}() on this plan")
        out = cls.alloc(*shape, *more)
        t = out.as_c()
        if not nodes:
            for n in cls._NODES:
                setattr(t, n, None)
        _check(fetch(self._h, C.byref(t)))
        return out

    def horizon(self, poses, row=None, seg_hint=None, window: int = 0, dt: float = 0.05, m_cap: int = 64,
                stream_ptr: int = 0) -> None:
        """Enqueue the horizon stage after the last trajectory() (rl_plan_horizon): locate the
        poses [Q, 2] on rows of that stage (row[q], None: row 0; within `window` segments of
        seg_hint[q], None or -1: anywhere) and resample up to m_cap ticks from there, dt apart,
        across the start line on a closed track.  As often as the caller likes without another
        run(); the trajectory stage stays as it is."""
        P, rw, hint = _hzn_query(poses, row, seg_hint, window, dt, m_cap)
        self._stage_enqueue("horizon", (P.shape[0], int(m_cap), float(dt)), stream_ptr, C.byref(_hzn_c(P, rw, hint, window, dt, m_cap)))

    def fetch_horizon(self) -> Horizon:
        """Download the last horizon() (rl_plan_fetch_horizon)."""
        return self._stage_fetch("horizon", True)

    def rejoin(self, poses, v0, cfg: RlCfg, row=None, seg_hint=None, window: int = 0, dt: float = 0.05,
               m_cap: int = 64, k_cap: int = 1024, stream_ptr: int = 0) -> None:
        """Enqueue the rejoin stage after the last trajectory() (rl_plan_rejoin): horizon()'s
        query with the car's speed v0 (a number or [Q]) and its limits now, cfg (one RlCfg, not
        necessarily the plan's).  The ticks follow the reachable speed profile from v0 until it
        meets the row's own, at most k_cap samples ahead.  The trajectory stage and the last
        horizon() stay as they are."""
        P, rw, hint, V0 = _rjn_query(poses, v0, cfg, row, seg_hint, window, dt, m_cap, k_cap)
        self._stage_enqueue("rejoin", (P.shape[0], int(m_cap), float(dt), int(k_cap)), stream_ptr,
                            C.byref(_rjn_c(P, rw, hint, V0, cfg, window, dt, m_cap, k_cap)))

    def fetch_rejoin(self, nodes: bool = True) -> Rejoin:
        """Download the last rejoin() (rl_plan_fetch_rejoin); nodes=False leaves node_v, node_t on
        the device."""
        out = self._stage_fetch("rejoin", nodes)
        out.set_k_lim(self.N, bool(self._keep[0].closed))
        return out

    def stop(self, poses, v0, cfg: RlCfg, stop_sample, v_target=None, row=None, seg_hint=None, window: int = 0,
             dt: float = 0.05, m_cap: int = 64, k_cap: int = 1024, stream_ptr: int = 0) -> None:
        """Enqueue the stop stage after the last trajectory() (rl_plan_stop): rejoin()'s query
        with a target, "do v_target (None: 0.0) at row sample stop_sample".  The ticks follow
        the march from v0 under the brake envelope of cfg up to the target, at most k_cap
        samples ahead.  The trajectory stage and the last horizon() and rejoin() stay as they
        are."""
        P, rw, hint, V0, J, VT = _stp_query(poses, v0, cfg, stop_sample, v_target, row, seg_hint, window, dt, m_cap, k_cap)
        self._stage_enqueue("stop", (P.shape[0], int(m_cap), float(dt), int(k_cap)), stream_ptr,
                            C.byref(_stp_c(P, rw, hint, V0, cfg, J, None if v_target is None else VT, window, dt, m_cap, k_cap)))

    def fetch_stop(self, nodes: bool = True) -> Stop:
        """Download the last stop() (rl_plan_fetch_stop); nodes=False leaves node_v, node_t, node_b
        on the device."""
        return self._stage_fetch("stop", nodes)

    def retime(self, poses, v0, cfg: RlCfg, row=None, seg_hint=None, window: int = 0, dt: float = 0.05,
               m_cap: int = 64, k_cap: int = 1024, stream_ptr: int = 0) -> None:
        """Enqueue the retime stage after the last trajectory() (rl_plan_retime): rejoin()'s query,
        answered with the speed profile of cfg (the car's limits now) over the k_cap samples
        ahead: the path stays, the speeds are recomputed under cfg from v0 and never exceed the
        row's.  The trajectory stage and the last horizon(), rejoin() and stop() stay as they
        are."""
        P, rw, hint, V0 = _rjn_query(poses, v0, cfg, row, seg_hint, window, dt, m_cap, k_cap)
        self._stage_enqueue("retime", (P.shape[0], int(m_cap), float(dt), int(k_cap)), stream_ptr,
                            C.byref(_rtm_c(P, rw, hint, V0, cfg, window, dt, m_cap, k_cap)))

    def fetch_retime(self, nodes: bool = True) -> Retime:
        """Download the last retime() (rl_plan_fetch_retime); nodes=False leaves node_v, node_t,
        node_b, node_c on the device."""
        return self._stage_fetch("retime", nodes)

    def recover(self, poses, v0, cfg: RlCfg, merge_len, dir_xy=None, row=None, seg_hint=None, window: int = 0,
                dt: float = 0.05, m_cap: int = 64, k_cap: int = 512, stream_ptr: int = 0) -> None:
        """Enqueue the recover stage after the last trajectory() and bounds() (rl_plan_recover):
        retime()'s query with a merge length (a number or [Q], metres along the row) and optionally
        the car's direction of travel dir_xy ([2] or [Q, 2]), answered with a path from the car's
        offset back to the row inside the bounds stage's free width and cfg's speed profile on
        it.  Every other stage stays as it is; a later bounds() invalidates it."""
        P, rw, hint, V0, D, H = _rcv_query(poses, v0, cfg, merge_len, dir_xy, row, seg_hint, window, dt, m_cap, k_cap)
        self._stage_enqueue("recover", (P.shape[0], int(m_cap), float(dt), int(k_cap)), stream_ptr,
                            C.byref(_rcv_c(P, rw, hint, V0, D, H, cfg, window, dt, m_cap, k_cap)))

    def fetch_recover(self, nodes: bool = True) -> Recover:
        """Download the last recover() (rl_plan_fetch_recover); nodes=False leaves the node arrays
        on the device."""
        return self._stage_fetch("recover", nodes)

    def recover_fan(self, poses, v0, cfg: RlCfg, merge_lens, dir_xy=None, row=None, seg_hint=None, window: int = 0,
                    dt: float = 0.05, m_cap: int = 64, k_cap: int = 512, stream_ptr: int = 0) -> None:
        """Enqueue the fan stage after the last trajectory() and bounds() (rl_plan_recover_fan):
        recover()'s query with C merge lengths per pose (merge_lens [C] or [Q, C]); every length is
        answered as recover() would, the candidates of a pose are ranked on the device in
        fan_order's order and the winner is served.  Every other stage stays as it is; a later
        bounds() invalidates it."""
        P, rw, hint, V0, D, H = _fan_query(poses, v0, cfg, merge_lens, dir_xy, row, seg_hint, window, dt, m_cap, k_cap)
        self._stage_enqueue("recover_fan", (P.shape[0], int(m_cap), float(dt), int(k_cap), D.shape[1]), stream_ptr,
                            C.byref(_fan_c(P, rw, hint, V0, D, H, cfg, window, dt, m_cap, k_cap)))

    def fetch_recover_fan(self, nodes: bool = True) -> RecoverFan:
        """Download the last recover_fan() (rl_plan_fetch_recover_fan): the winner's fields, best
        and the candidates' table; nodes=False leaves the node arrays on the device."""
        return self._stage_fetch("recover_fan", nodes)

    def bounds(self, veh_width: Optional[float] = None, margin: Optional[float] = None, stream_ptr: int = 0) -> None:
        """Enqueue the bounds stage after the last trajectory() (rl_plan_bounds): the free track
        width lo, hi along the unit normal of every sample of that stage's rows, row for row, with
        guard = veh_width / 2 + margin (None: the problem's veh_width, the safety_margin_m of the
        plan's first cfg).  Every other stage stays as it is."""
        w, m = _bnd_guard(self._keep[0].veh_width if veh_width is None else veh_width,
                          self._keep[1][0].safety_margin_m if margin is None else margin)
        self._shapes["horizon_bounds"] = None
        self._stage_enqueue("bounds", (self._shapes.get("trajectory") or ())[:2], stream_ptr, C.byref(abi.RlBndQuery(w, m)))

    def fetch_bounds(self) -> Bounds:
        """Download the last bounds() (rl_plan_fetch_bounds): Bounds(lo, hi, nx, ny), [R, N] each."""
        return self._stage_fetch("bounds")

    def horizon_bounds(self, stream_ptr: int = 0) -> None:
        """Enqueue the bounds at the ticks of the last horizon() (rl_plan_horizon_bounds), from
        the last bounds() of the same trajectory(); nothing is uploaded."""
        self._stage_enqueue("horizon_bounds", (self._shapes.get("horizon") or ())[:2], stream_ptr)

    def fetch_horizon_bounds(self) -> HorizonBounds:
        """Download the last horizon_bounds() (rl_plan_fetch_horizon_bounds)."""
        return self._stage_fetch("horizon_bounds")

    def rollouts(self, xy, v=None, row=None, seg_hint=None, window0: int = 0, window: int = 8, weights=ROLLOUT_WEIGHTS,
                 hard_bounds: bool = False, group_size: Optional[int] = None, k: int = 1, stream_ptr: int = 0) -> None:
        """Enqueue the rollout stage after the last trajectory() and bounds() (rl_plan_rollouts): the
        rollouts xy [Q, T, 2] (speeds v [Q, T], optional) are located pose by pose on rows of the
        trajectory stage (row[q], None: row 0), pose 0 within window0 of seg_hint[q] (None or -1:
        anywhere), every later pose within `window` of the segment found for the pose before it;
        each rollout is scored with weights = (w_e, w_out, w_v, w_prog) and the k best of every
        group of group_size (None: all Q) are ranked on the device.  As often as the caller likes
        without another run(); every other stage stays as it is; a later bounds() invalidates it."""
        qy = _rll_query(xy, v, row, seg_hint, window0, window, weights, hard_bounds, group_size, k)
        self._stage_enqueue("rollouts", qy[0].shape[:2] + (qy[0].shape[0] // qy[8], qy[9]), stream_ptr, C.byref(_rll_c(qy)))

    def fetch_rollouts(self, poses: bool = False) -> Rollouts:
        """Download the last rollouts() (rl_plan_fetch_rollouts): the per-rollout values and order;
        poses=True brings the per-pose arrays down as well."""
        return self._stage_fetch("rollouts", True, poses)

    def device_outputs(self, which: int) -> abi.RlOut:
        d = abi.RlOut()
        _check(_lib().rl_plan_device_outputs(self._h, which, C.byref(d)))
        return d

    def bind_device_outputs(self, which: int, ptrs: dict) -> None:
        """Use caller-owned device buffers (name -> device pointer int, e.g. a
        torch tensor's data_ptr()) as result storage for mode `which`."""
        d = abi.RlOut()
        for name, ptr in ptrs.items():
            typ = C.POINTER(C.c_int32) if name in ("evals", "accepts", "vpass_sweeps") else C.POINTER(C.c_double)
            setattr(d, name, C.cast(C.c_void_p(ptr), typ))
        _check(_lib().rl_plan_bind_device_outputs(self._h, which, C.byref(d)))

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib().rl_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------- reference-shaped calls
def _single(center, innerE, outerE, veh_width, L, closed, cfg, mincurv):
    cfg = cfg if cfg is not None else default_cfg()
    prob = Problem(center=center, L=L, inner_seg=innerE, outer_seg=outerE, veh_width=veh_width, closed=closed)
    if prob.N == 0:                       # ref:689 / 912: N==0 -> empty Result
        z = np.zeros(0)
        if mincurv:
            return MinCurvResult(np.zeros((0, 2)), z, z, z, z)
        return MinTimeResult(np.zeros((0, 2)), z, z, z, z, v=z, ax=z, lap_time=0.0)
    mc, mt = optimize_batch(prob, cfg, None, 1, mincurv=mincurv, mintime=not mincurv)
    o = mc if mincurv else mt
    res = dict(raceline=np.stack([o.x[0], o.y[0]], axis=1), heading=o.heading[0], curvature=o.kappa[0],
               alpha_total=o.alpha_total[0], alpha_last=o.alpha_last[0], evals=o.evals[0])
    if mincurv:
        return MinCurvResult(**res)
    return MinTimeResult(**res, v=o.v[0], ax=o.ax[0], lap_time=float(o.lap[0]), vpass_sweeps=o.vpass_sweeps[0])


def compute_min_curvature_raceline(center, innerE, outerE, veh_width: float, L: float, closed: bool,
                                   cfg: Optional[RlCfg] = None) -> MinCurvResult:
    """raceline_min_curv::compute_min_curvature_raceline (ref:683)."""
    return _single(center, innerE, outerE, veh_width, L, closed, cfg, True)


def compute_min_time_raceline(center, innerE, outerE, veh_width: float, L: float, closed: bool,
                              cfg: Optional[RlCfg] = None) -> MinTimeResult:
    """raceline_min_time::compute_min_time_raceline (ref:905)."""
    return _single(center, innerE, outerE, veh_width, L, closed, cfg, False)


# ------------------------------------------------------------- CSV writers
def _f9(x: float) -> str:
    """std::fixed + precision(9) (ref:1354)."""
    return f"{x:.9f}"


def _vkappa(kappa: float, cfg: RlCfg) -> float:
    """v_kappa column (ref:1369-1370): min(v_cap, sqrt(a_lat_max / max(|k|, kappa_eps)))."""
    k = abs(float(kappa))
    denom = cfg.kappa_eps if k < cfg.kappa_eps else k          # std::max(|k|, eps)
    v = float(np.sqrt(cfg.a_lat_max / denom))
    return cfg.v_cap_mps if v > cfg.v_cap_mps else v


def _s_rel(s0: float, L: float, k: int, n: int) -> float:
    """si - s0 with si = s0 + L*(k/max(1,n)) (ref:1367-1368), same roundings."""
    return (s0 + L * (float(k) / float(max(1, n)))) - s0


def write_raceline_csvs(base: str, res: MinCurvResult, L: float, cfg: Optional[RlCfg] = None,
                        emit_closed_duplicate: bool = True, s0: float = 0.0) -> None:
    """Writers of pipeline::compute_raceline_and_save (ref:1351-1382)."""
    cfg = cfg if cfg is not None else default_cfg()
    P = res.raceline
    with open(base + "_raceline.csv", "w") as f:
        for x, y in P:
            f.write(f"{_f9(x)},{_f9(y)}\n")
        if emit_closed_duplicate and len(P):
            f.write(f"{_f9(P[0, 0])},{_f9(P[0, 1])}\n")
    with open(base + "_raceline_with_geom.csv", "w") as f:
        f.write("s,x,y,heading_rad,curvature,alpha_last,v_kappa_mps\n")
        n = len(P)
        for k in range(n):
            s = _s_rel(s0, L, k, n)
            f.write(",".join(_f9(v) for v in (s, P[k, 0], P[k, 1], res.heading[k], res.curvature[k],
                                                 res.alpha_last[k], _vkappa(res.curvature[k], cfg))) + "\n")
        if emit_closed_duplicate and n:
            f.write(",".join(_f9(v) for v in (L, P[0, 0], P[0, 1], res.heading[0], res.curvature[0],
                                                 res.alpha_last[0], _vkappa(res.curvature[0], cfg))) + "\n")


def write_mintime_csvs(base: str, res: MinTimeResult, L: float, emit_closed_duplicate: bool = True,
                       s0: float = 0.0) -> None:
    """Writers of pipeline::compute_mintime_and_save (ref:1400-1436)."""
    P = res.raceline
    with open(base + "_mintime_raceline.csv", "w") as f:
        for x, y in P:
            f.write(f"{_f9(x)},{_f9(y)}\n")
        if emit_closed_duplicate and len(P):
            f.write(f"{_f9(P[0, 0])},{_f9(P[0, 1])}\n")
    with open(base + "_mintime_with_geom.csv", "w") as f:
        f.write("s,x,y,heading_rad,curvature,alpha_last,v_mps,ax_mps2\n")
        n = len(P)
        for k in range(n):
            s = _s_rel(s0, L, k, n)
            f.write(",".join(_f9(v) for v in (s, P[k, 0], P[k, 1], res.heading[k], res.curvature[k],
                                                 res.alpha_last[k], res.v[k], res.ax[k])) + "\n")
        if emit_closed_duplicate and n:
            f.write(",".join(_f9(v) for v in (L, P[0, 0], P[0, 1], res.heading[0], res.curvature[0],
                                                 res.alpha_last[0], res.v[0], res.ax[0])) + "\n")


def compute_raceline_and_save(base: str, center_for_opt, s0: float, L: float, closed: bool, inner_from_mids,
                              outer_from_mids, cfg: Optional[RlCfg] = None) -> MinCurvResult:
    """pipeline::compute_raceline_and_save (ref:1337-1383)."""
    cfg = cfg if cfg is not None else default_cfg()
    res = compute_min_curvature_raceline(center_for_opt, edges_for(inner_from_mids, closed),
                                         edges_for(outer_from_mids, closed), cfg.veh_width_m, L, closed, cfg)
    write_raceline_csvs(base, res, L, cfg, s0=s0)
    return res


def compute_mintime_and_save(base: str, center_for_opt, s0: float, L: float, closed: bool, inner_from_mids,
                             outer_from_mids, cfg: Optional[RlCfg] = None, debug_dump: bool = True,
                             device: int = 0) -> MinTimeResult:
    """pipeline::compute_mintime_and_save (ref:1385-1593).  debug_dump (cfg::debug_dump,
    on by default in the reference, ref:117) adds the centreline / min-curvature lap
    evaluations and <base>_debug_compare_paths.csv (debug_dump())."""
    import sys
    cfg = cfg if cfg is not None else default_cfg()
    res = compute_min_time_raceline(center_for_opt, edges_for(inner_from_mids, closed),
                                    edges_for(outer_from_mids, closed), cfg.veh_width_m, L, closed, cfg)
    write_mintime_csvs(base, res, L, s0=s0)
    sys.stderr.write(f"[mintime] Estimated laptime: {res.lap_time:.3f} s\n")
    if debug_dump:
        debug_dump_block(base, center_for_opt, s0, L, closed, res, cfg, device)
    return res


# --------------------------------------------------- lap evaluation (§8f row 2)
def lap_eval(paths, L, closed: bool, cfg: Optional[RlCfg] = None, device: int = 0, return_ms: bool = False):
    """B lap evaluations on the GPU (rl_lap_eval): heading/curvature with h = L[b]/N and
    velocity_profile_forward_backward on path b (ref:1045-1048, 1466-1478).
    paths [B, N, 2]; returns min-time Outputs (heading, kappa, v, ax, lap, sweeps)."""
    P = np.ascontiguousarray(paths, dtype=np.float64)
    if P.ndim == 2:
        P = P[None]
    B, N = P.shape[0], P.shape[1]
    Ls = np.ascontiguousarray(np.broadcast_to(np.asarray(L, dtype=np.float64), (B,)))
    cfg = cfg if cfg is not None else default_cfg()
    out = Outputs.alloc(B, N, 0, True)         # max_outer_iters = 0: vpass_sweeps [B][1]
    o = out.as_c()
    o.evals = None
    o.accepts = None
    arr, n = abi.cfg_array(cfg)
    ms = C.c_float(0.0)
    rc = _lib().rl_lap_eval(abi.dptr(P), abi.dptr(Ls), N, B, 1 if closed else 0, arr, n, int(device), C.byref(o),
                            C.byref(ms))
    _check(rc)
    out.x, out.y = P[:, :, 0].copy(), P[:, :, 1].copy()
    return (out, float(ms.value)) if return_ms else out


_LIBM = None


def _hypot(a: float, b: float) -> float:
    """glibc hypot (what std::hypot resolves to in the reference build)."""
    global _LIBM
    if _LIBM is None:
        _LIBM = C.CDLL("libm.so.6")
        _LIBM.hypot.restype = C.c_double
        _LIBM.hypot.argtypes = [C.c_double, C.c_double]
    return _LIBM.hypot(a, b)


def path_length(P, closed: bool) -> float:
    """The debug dump's path_length lambda (ref:1443-1448)."""
    P = np.asarray(P, dtype=np.float64)
    n = len(P)
    if n <= 1:
        return 0.0
    tot = 0.0
    for i in range(n - 1):
        tot += _hypot(P[i + 1, 0] - P[i, 0], P[i + 1, 1] - P[i, 1])
    if closed and n >= 2:
        tot += _hypot(P[0, 0] - P[n - 1, 0], P[0, 1] - P[n - 1, 1])
    return tot


def normals_from_points(P, closed: bool) -> np.ndarray:
    """normals_from_points_generic (ref:581-593) restated on the host."""
    P = np.asarray(P, dtype=np.float64)
    N = len(P)
    n = np.zeros((N, 2))
    for i in range(N):
        if N == 1:
            tx, ty = 1.0, 0.0
        elif closed:
            ip, im = (i + 1) % N, (i - 1 + N) % N
            tx, ty = (P[ip, 0] - P[im, 0]) * 0.5, (P[ip, 1] - P[im, 1]) * 0.5
        elif i == 0:
            tx, ty = P[1, 0] - P[0, 0], P[1, 1] - P[0, 1]
        elif i == N - 1:
            tx, ty = P[N - 1, 0] - P[N - 2, 0], P[N - 1, 1] - P[N - 2, 1]
        else:
            tx, ty = (P[i + 1, 0] - P[i - 1, 0]) * 0.5, (P[i + 1, 1] - P[i - 1, 1]) * 0.5
        if float(np.sqrt(tx * tx + ty * ty)) < 1e-15:
            tx, ty = 1.0, 0.0
        vx, vy = -ty, tx
        nn = float(np.sqrt(vx * vx + vy * vy))
        if not (nn < 1e-15):
            n[i] = (vx / nn, vy / nn)
    return n


DEBUG_HEADER = ("s,cx,cy,mt_x,mt_y,mc_x,mc_y,d_mt_signed_m,d_mc_signed_m,"
                "d_mt_abs_m,d_mc_abs_m,kappa_mt,v_mt,ax_mt,alat_mt,alat_ratio,"
                "gamma,a_acc_cap,a_brk_cap,a_power_cap\n")


def debug_compare_rows(center, s0: float, L: float, res_mt: "MinTimeResult", mc_path, cfg: RlCfg,
                       closed: bool) -> np.ndarray:
    """Rows of <base>_debug_compare_paths.csv (ref:1490-1561), same operations in the
    same order, libstdc++ min/max/clamp forms."""
    smax = lambda a, b: b if a < b else a          # noqa: E731  std::max
    smin = lambda a, b: b if b < a else a          # noqa: E731  std::min
    nan = float("nan")
    center = np.asarray(center, dtype=np.float64)
    Pmt = np.asarray(res_mt.raceline, dtype=np.float64)
    mc = np.asarray(mc_path, dtype=np.float64).reshape(-1, 2) if mc_path is not None else np.zeros((0, 2))
    nc = normals_from_points(center, closed)
    N = min(len(Pmt), len(center))
    rows = np.zeros((N, 20))
    c = cfg
    for k in range(N):
        si = s0 + L * (float(k) / float(max(1, N)))
        cx, cy = center[k]
        mx, my = Pmt[k]
        if len(mc) > k:
            ccx, ccy = mc[k]
        else:
            ccx = ccy = nan
        dmt = (mx - cx) * nc[k, 0] + (my - cy) * nc[k, 1]
        dmc = (ccx - cx) * nc[k, 0] + (ccy - cy) * nc[k, 1] if np.isfinite(ccx) else nan
        admt = abs(dmt)
        admc = abs(dmc) if np.isfinite(dmc) else nan
        kap = float(res_mt.curvature[k]) if k < len(res_mt.curvature) else 0.0
        v = float(res_mt.v[k]) if k < len(res_mt.v) else 0.0
        ax = float(res_mt.ax[k]) if k < len(res_mt.ax) else 0.0
        alat = v * v * abs(kap)
        alat_ratio = smin(1.0, alat / c.a_total_max) if c.a_total_max > 1e-9 else 0.0
        vkappa = float(np.sqrt(c.a_lat_max / smax(abs(kap), c.kappa_eps)))
        x = (vkappa - v) / smax(1e-6, vkappa)
        pen = 0.0 if x < 0 else (1.0 if x > 1 else x)
        gamma = 1.0 + c.w_time_gain * pen
        alatloc = v * v * abs(kap)
        a_res = float(np.sqrt(smax(0.0, c.a_total_max * c.a_total_max - alatloc * alatloc)))
        Fd = 0.5 * c.rho_air * c.Cd * c.A_front_m2 * v * v
        Fr = c.mass_kg * 9.81 * c.c_rr
        a_power = (c.P_max_W / (c.mass_kg * v) - (Fd + Fr) / c.mass_kg) if (c.P_max_W > 0 and v > 1e-6) else 1e9
        m3 = a_res                                     # std::min({a_res, acc_cap, a_power})
        if c.a_long_acc_cap < m3:
            m3 = c.a_long_acc_cap
        if a_power < m3:
            m3 = a_power
        a_acc = smax(0.0, m3)
        a_brk = smax(0.0, smin(a_res, c.a_long_brake_cap) + (Fd + Fr) / c.mass_kg)
        a_pow = smax(0.0, a_power)
        rows[k] = (si - s0, cx, cy, mx, my, ccx, ccy, dmt, dmc, admt, admc, kap, v, ax, alat, alat_ratio,
                   gamma, a_acc, a_brk, a_pow)
    return rows


def format_debug_compare_csv(rows: np.ndarray) -> str:
    out = [DEBUG_HEADER]
    for r in np.asarray(rows, dtype=np.float64).reshape(-1, 20):
        out.append(",".join(_f9(v) for v in r) + "\n")
    return "".join(out)


def debug_dump_block(base: str, center_for_opt, s0: float, L: float, closed: bool, res_mt: "MinTimeResult",
               cfg: RlCfg, device: int = 0, debug_offset_warn_m: float = 0.04, log=None) -> dict:
    """The cfg::debug_dump block of compute_mintime_and_save (ref:1441-1593): centreline
    and min-curvature laps with the same dynamics (two GPU lap evaluations), and
    <base>_debug_compare_paths.csv.  The min-curvature path is re-read from
    <base>_raceline.csv as the reference does (ref:1452-1459)."""
    import sys
    log = log if log is not None else sys.stderr
    center = np.asarray(center_for_opt, dtype=np.float64).reshape(-1, 2)
    mc = load_csv_xy(base + "_raceline.csv") if os.path.exists(base + "_raceline.csv") else np.zeros((0, 2))
    if len(mc) and closed and len(mc) >= 2 and abs(mc[0, 0] - mc[-1, 0]) <= 1e-12 and abs(mc[0, 1] - mc[-1, 1]) <= 1e-12:
        mc = mc[:-1]
    Nc = len(center)
    laps = {}
    if Nc:
        paths, Ls = [center], [L]
        if len(mc) == Nc:
            paths.append(mc)
            Ls.append(path_length(mc, closed))
        ev = lap_eval(np.stack(paths), np.array(Ls), closed, cfg, device)
        laps["center"] = float(ev.lap[0])
        if len(paths) == 2:
            laps["mincurv"] = float(ev.lap[1])
        elif len(mc):
            laps["mincurv"] = float(lap_eval(mc, [path_length(mc, closed)], closed, cfg, device).lap[0])
    lap_c = laps.get("center", 0.0)
    if "mincurv" in laps:
        log.write(f"[debug] centerline lap ≈ {lap_c:.3f} s,  min-curv lap ≈ {laps['mincurv']:.3f} s,  "
                  f"min-time lap ≈ {res_mt.lap_time:.3f} s\n")
    else:
        log.write(f"[debug] centerline lap ≈ {lap_c:.3f} s,  (min-curv not found),  min-time lap ≈ {res_mt.lap_time:.3f} s\n")
    rows = debug_compare_rows(center, s0, L, res_mt, mc if len(mc) else None, cfg, closed)
    with open(base + "_debug_compare_paths.csv", "w") as f:
        f.write(format_debug_compare_csv(rows))
    N = len(rows)
    admt, admc = rows[:, 9], rows[:, 10]
    stats = {"laps": laps, "mean_abs_mt": float(np.sum(admt) / max(1, N)) if N else 0.0,
             "max_abs_mt": float(np.max(admt)) if N else 0.0,
             "near_cnt": int(np.sum(admt < debug_offset_warn_m))}
    log.write(f"[debug] min-time vs center: mean|offset|={stats['mean_abs_mt']:.3f} m, "
              f"max={stats['max_abs_mt']:.3f} m, within {debug_offset_warn_m:.3f} m : {stats['near_cnt']}/{N}\n")
    if "mincurv" in laps and laps["mincurv"] > 0:
        log.write(f"[debug] lap gain vs min-curv: {(laps['mincurv'] - res_mt.lap_time) / laps['mincurv'] * 100.0:.3f} %\n")
    return stats


# ------------------------------------------------------- step 6: geometry
GEOM_HEADER = "s,x,y,heading_rad,curvature,dist_to_inner,dist_to_outer,width,v_kappa_mps\n"


def format_geom_csv(rows: np.ndarray) -> str:
    """<base>_with_geom.csv text of pipeline::compute_geom_and_save (ref:1300-1334):
    header, then every row with std::fixed / precision(9)."""
    out = [GEOM_HEADER]
    for r in np.asarray(rows, dtype=np.float64).reshape(-1, 9):
        out.append(",".join(_f9(v) for v in r) + "\n")
    return "".join(out)


def corridor(prob: Problem, cfg: Optional[RlCfg] = None, device: int = 0):
    """The optimisers' first corridor (ref:692-711) of the path prob.center on the GPU
    (rl_corridor): normals, then lo/hi per sample with guard = veh_width/2 + margin."""
    cfg = cfg if cfg is not None else default_cfg()
    N = prob.N
    lo, hi = np.zeros(max(N, 1)), np.zeros(max(N, 1))
    p = prob.as_c()
    _check(_lib().rl_corridor(C.byref(p), C.byref(cfg), int(device), abi.dptr(lo), abi.dptr(hi)))
    return lo[:N], hi[:N]


def compute_geom(gp: GeomProblem, cfg: Optional[RlCfg] = None, device: int = 0, return_ms: bool = False):
    """Rows of pipeline::compute_geom_and_save (ref:1295-1335) on the GPU (rl_geom):
    [Kmax + emit_closed_duplicate, 9] = s_rel, x, y, heading, curvature, d_in, d_out,
    width, v_kappa.  Fails loudly without a device (no CPU path)."""
    lib = _lib()
    cfg = cfg if cfg is not None else default_cfg()
    rows = np.zeros((max(gp.rows, 1), 9))
    g = gp.as_c()
    ms = C.c_float(0.0)
    n = lib.rl_geom(C.byref(g), C.byref(cfg), int(device), rows.ctypes.data_as(C.POINTER(C.c_double)),
                    C.byref(ms))
    if n < 0:
        raise RacelineError(n, lib.rl_last_error().decode())
    rows = rows[:n]
    return (rows, float(ms.value)) if return_ms else rows


def compute_geom_and_save(base: str, gp: GeomProblem, cfg: Optional[RlCfg] = None, device: int = 0) -> np.ndarray:
    """pipeline::compute_geom_and_save (ref:1288-1335): writes <base>_with_geom.csv."""
    rows = compute_geom(gp, cfg, device)
    with open(base + "_with_geom.csv", "w") as f:
        f.write(format_geom_csv(rows))
    return rows


# ------------------------------------------------- CSV number format (§8f row 3)
def format_table(table, device: int = 0, return_offsets: bool = False):
    """glibc "%.9f" CSV rows ("v,...,v\\n") of a [rows, cols] table, formatted on the GPU
    (rl_format_csv); byte-identical to the reference's std::fixed/precision(9) output."""
    T = np.ascontiguousarray(table, dtype=np.float64)
    if T.ndim == 1:
        T = T[:, None]
    rows, cols = T.shape
    cap = rows * cols * 22
    buf = C.create_string_buffer(max(cap, 1))
    n = C.c_int64(0)
    offs = np.zeros(rows + 1, dtype=np.int64)
    rc = _lib().rl_format_csv(abi.dptr(T), rows, cols, int(device), C.cast(buf, C.c_void_p), cap, C.byref(n),
                              offs.ctypes.data_as(C.POINTER(C.c_int64)))
    _check(rc)
    text = buf.raw[: n.value]
    return (text, offs) if return_offsets else text


def write_batch_raceline_with_geom(bases, mc: Outputs, L: float, cfg: Optional[RlCfg] = None, s0: float = 0.0,
                                   emit_closed_duplicate: bool = True, device: int = 0) -> None:
    """<base_b>_raceline_with_geom.csv (ref:1362-1381) for all B instances of a batch in
    one GPU formatting pass (rows split by the returned offsets)."""
    cfg = cfg if cfg is not None else default_cfg()
    B, N = mc.x.shape
    s = np.array([_s_rel(s0, L, k, N) for k in range(N)])
    vk = lambda kap: np.array([_vkappa(k, cfg) for k in kap])          # noqa: E731
    per = N + (1 if (emit_closed_duplicate and N) else 0)
    T = np.zeros((B, per, 7))
    for b in range(B):
        T[b, :N] = np.stack([s, mc.x[b], mc.y[b], mc.heading[b], mc.kappa[b], mc.alpha_last[b], vk(mc.kappa[b])], 1)
        if per > N:
            T[b, N] = (L, *T[b, 0, 1:])
    text, offs = format_table(T.reshape(B * per, 7), device, return_offsets=True)
    head = b"s,x,y,heading_rad,curvature,alpha_last,v_kappa_mps\n"
    for b, base in enumerate(bases):
        with open(base + "_raceline_with_geom.csv", "wb") as f:
            f.write(head + text[offs[b * per]: offs[(b + 1) * per]])


def load_csv_xy(path: str) -> np.ndarray:
    """io::loadCSV_XY (ref:267-279): x,y per line; ',' ';' tab or space."""
    pts = []
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            parts = line.replace(";", " ").replace("\t", " ").replace(",", " ").split()
            if len(parts) >= 2:
                try:
                    pts.append((float(parts[0]), float(parts[1])))
                except ValueError:
                    continue
    return np.array(pts, dtype=np.float64).reshape(-1, 2)


def seeds_range(B: int, first: int = 0) -> np.ndarray:
    """Seeds first..first+B-1 (seed 0 = the reference's α≡0 start)."""
    return np.arange(first, first + B, dtype=np.uint64)


__all__ = ["RacelineError", "MinCurvResult", "MinTimeResult", "Plan", "Problem", "RlCfg", "Outputs",
           "default_cfg", "set_mu", "ring_edges", "polyline_edges", "edges_for", "optimize_batch",
           "optimize_best", "rank_scores", "Selected", "path_lengths", "path_length", "lap_eval",
           "compute_min_curvature_raceline", "compute_min_time_raceline", "compute_raceline_and_save",
           "compute_mintime_and_save", "write_raceline_csvs", "write_mintime_csvs", "load_csv_xy",
           "seeds_range", "Trajectory", "trajectory", "trajectory_host", "best_trajectory"]
