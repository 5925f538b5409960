"""ctypes mirror of ``include/rl_abi.h`` (the C-ABI drop-in boundary).

The structs here are byte-for-byte the C structs of ``rl_abi.h``; the loader
binds ``librl.so`` (HIP kernels for gfx950 + the C-ABI).  There is no CPU
fallback: if the library is missing, :func:`load_library` raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import weakref
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "_lib", "librl.so")
# experiment builds only (scripts/build_variants.py): RL_LIB names another librl.so to load
if os.environ.get("RL_LIB"):
    LIB_PATH = os.path.abspath(os.environ["RL_LIB"])

RL_OK = 0
RL_EINVAL = -1
RL_ENODEV = -2
RL_EHIP = -3
RL_ENOMEM = -4
RL_ETOOBIG = -5

RL_MODE_MINCURV = 1
RL_MODE_MINTIME = 2
RL_SEED_SIGMA = 0.25


class RlCfg(C.Structure):
    """``rl_cfg`` — hot-path subset of ``cfg::Config`` (main.cpp:47-119)."""

    _fields_ = [
        ("veh_width_m", C.c_double),
        ("safety_margin_m", C.c_double),
        ("lambda_smooth", C.c_double),
        ("max_outer_iters", C.c_int32),
        ("max_inner_iters", C.c_int32),
        ("step_init", C.c_double),
        ("step_min", C.c_double),
        ("armijo_c", C.c_double),
        ("kappa_eps", C.c_double),
        ("v_cap_mps", C.c_double),
        ("mass_kg", C.c_double),
        ("Cd", C.c_double),
        ("A_front_m2", C.c_double),
        ("rho_air", C.c_double),
        ("c_rr", C.c_double),
        ("P_max_W", C.c_double),
        ("mu", C.c_double),
        ("a_total_max", C.c_double),
        ("a_lat_max", C.c_double),
        ("a_long_acc_cap", C.c_double),
        ("a_long_brake_cap", C.c_double),
        ("w_time_gain", C.c_double),
        ("time_gamma_power", C.c_double),
        ("time_weight_use_inv_v", C.c_int32),
        ("max_vpass_iters", C.c_int32),
        ("inv_v_gain", C.c_double),
        ("use_total_ge_lat", C.c_int32),
        ("_pad0", C.c_int32),
    ]

    def to_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_ if not n.startswith("_")}

    @classmethod
    def from_dict(cls, d: dict) -> "RlCfg":
        c = cls()
        for n, t in cls._fields_:
            if n in d:
                setattr(c, n, d[n])
        return c


class RlProblem(C.Structure):
    _fields_ = [
        ("center_xy", C.POINTER(C.c_double)),
        ("N", C.c_int32),
        ("closed", C.c_int32),
        ("L", C.c_double),
        ("inner_seg", C.POINTER(C.c_double)),
        ("Ei", C.c_int32),
        ("Eo", C.c_int32),
        ("outer_seg", C.POINTER(C.c_double)),
        ("veh_width", C.c_double),
    ]


class RlOut(C.Structure):
    _fields_ = [
        ("x", C.POINTER(C.c_double)),
        ("y", C.POINTER(C.c_double)),
        ("heading", C.POINTER(C.c_double)),
        ("kappa", C.POINTER(C.c_double)),
        ("alpha_total", C.POINTER(C.c_double)),
        ("alpha_last", C.POINTER(C.c_double)),
        ("v", C.POINTER(C.c_double)),
        ("ax", C.POINTER(C.c_double)),
        ("lap", C.POINTER(C.c_double)),
        ("evals", C.POINTER(C.c_int32)),
        ("accepts", C.POINTER(C.c_int32)),
        ("vpass_sweeps", C.POINTER(C.c_int32)),
    ]


RL_SELECT_MAX_K = 64
RL_ABI_MINOR = 1
RL_SCORE_DEFAULT = 0      # lap for min-time, h * sum kappa^2 for min-curvature
RL_SCORE_LAP = 1          # the lap stage's lap (differs from the default for min-curvature only)


class RlSelect(C.Structure):
    """``rl_select`` — which mode's results are ranked, winners per group, group size (0 = B)."""

    _fields_ = [("mode", C.c_int32), ("k", C.c_int32), ("group_size", C.c_int32), ("_pad", C.c_int32)]


RL_FEATURE_TRAJECTORY = 1  # rl_abi_features() bit 0: the trajectory stage
RL_TRAJ_ALL = 0            # one trajectory per instance
RL_TRAJ_SELECTED = 1       # one per winner of the plan's valid selection
RL_TRAJ_MAX_TICKS = 1 << 20
TRAJ_COLS = ("s", "x", "y", "heading", "kappa", "v", "ax")


class RlTraj(C.Structure):
    """``rl_traj`` — caller-allocated trajectory arrays: the columns [R][M_cap], stamps [R][N+1],
    T [R], count [R]; NULL fields are skipped."""

    _fields_ = [(n, C.POINTER(C.c_double)) for n in TRAJ_COLS + ("stamps", "T")] + [("count", C.POINTER(C.c_int32))]


RL_FEATURE_HORIZON = 2     # rl_abi_features() bit 1: the horizon stage
RL_HZN_MAX_QUERIES = 65536
HZN_LOC = ("u", "t0", "s0", "e", "dist2")


class RlHznQuery(C.Structure):
    """``rl_hzn_query`` — Q poses [Q][2] with their rows and segment hints (NULL: row 0, no hint)."""

    _fields_ = [("pose_xy", C.POINTER(C.c_double)), ("row", C.POINTER(C.c_int32)), ("seg_hint", C.POINTER(C.c_int32)),
                ("Q", C.c_int32), ("window", C.c_int32), ("M_cap", C.c_int32), ("_pad", C.c_int32), ("dt", C.c_double)]


class RlHzn(C.Structure):
    """``rl_hzn`` — caller-allocated horizon arrays: the columns [Q][M_cap], u, t0, s0, e, dist2 [Q],
    seg and count [Q]; NULL fields are skipped."""

    _fields_ = [(n, C.POINTER(C.c_double)) for n in TRAJ_COLS + HZN_LOC] + [(n, C.POINTER(C.c_int32)) for n in ("seg", "count")]


RL_FEATURE_REJOIN = 4      # rl_abi_features() bit 2: the rejoin stage
RL_RJN_MAX_NODES = 1024
RJN_SCAL = ("t_merge", "t_loss")
RJN_INTS = ("seg", "count", "merge_node", "overspeed")
RJN_NODES = ("node_v", "node_t")


class RlRjnQuery(C.Structure):
    """``rl_rjn_query`` — ``rl_hzn_query`` plus the car's speeds v0 [Q], one ``rl_cfg`` (the car's
    limits now) and the number of march nodes K_cap."""

    _fields_ = RlHznQuery._fields_ + [("v0", C.POINTER(C.c_double)), ("cfg", C.POINTER(RlCfg)), ("K_cap", C.c_int32),
                                      ("_pad2", C.c_int32)]


class RlRjn(C.Structure):
    """``rl_rjn`` — ``rl_hzn`` plus merge_node, overspeed, t_merge, t_loss [Q] and the optional
    march nodes node_v, node_t [Q][K_cap + 1]; NULL fields are skipped."""

    _fields_ = (RlHzn._fields_ + [(n, C.POINTER(C.c_int32)) for n in RJN_INTS[2:]] +
                [(n, C.POINTER(C.c_double)) for n in RJN_SCAL + RJN_NODES])


RL_FEATURE_STOP = 8        # rl_abi_features() bit 3: the stop stage
STP_SCAL = ("t_stop", "v_end", "s_stop", "v_excess")
STP_INTS = ("seg", "count", "stop_node", "overspeed", "reachable", "brake_node")
STP_NODES = ("node_v", "node_t", "node_b")


class RlStpQuery(C.Structure):
    """``rl_stp_query`` — one ``rl_rjn_query`` plus the target samples stop_sample [Q] and the
    speeds to have there v_target [Q] (NULL: all 0.0)."""

    _fields_ = [("rj", RlRjnQuery), ("stop_sample", C.POINTER(C.c_int32)), ("v_target", C.POINTER(C.c_double))]


class RlStp(C.Structure):
    """``rl_stp`` — ``rl_rjn``'s layout with stop_node, overspeed, t_stop, v_end in the place of
    its four, then reachable, brake_node, s_stop, v_excess [Q] and the optional node_b
    [Q][K_cap + 1]; NULL fields are skipped."""

    _fields_ = (RlHzn._fields_ + [(n, C.POINTER(C.c_int32)) for n in STP_INTS[2:4]] +
                [(n, C.POINTER(C.c_double)) for n in STP_SCAL[:2] + STP_NODES[:2]] +
                [(n, C.POINTER(C.c_int32)) for n in STP_INTS[4:]] +
                [(n, C.POINTER(C.c_double)) for n in STP_SCAL[2:] + STP_NODES[2:]])


RL_FEATURE_RETIME = 32     # rl_abi_features() bit 5: the retime stage
RTM_SCAL = ("t_end", "t_loss", "v_excess")
RTM_INTS = ("seg", "count", "end_node", "overspeed", "feasible", "bind_node")
RTM_NODES = ("node_v", "node_t", "node_b", "node_c")


class RlRtmQuery(C.Structure):
    """``rl_rtm_query`` — one ``rl_rjn_query``: the pose, the car's speed and its limits now."""

    _fields_ = [("rj", RlRjnQuery)]


class RlRtm(C.Structure):
    """``rl_rtm`` — ``rl_rjn``'s layout with end_node, overspeed, t_end, t_loss in the place of its
    four, then feasible, bind_node, v_excess [Q] and the optional node_b, node_c [Q][K_cap + 1];
    NULL fields are skipped."""

    _fields_ = (RlHzn._fields_ + [(n, C.POINTER(C.c_int32)) for n in RTM_INTS[2:4]] +
                [(n, C.POINTER(C.c_double)) for n in RTM_SCAL[:2] + RTM_NODES[:2]] +
                [(n, C.POINTER(C.c_int32)) for n in RTM_INTS[4:]] +
                [(n, C.POINTER(C.c_double)) for n in RTM_SCAL[2:] + RTM_NODES[2:]])


RL_FEATURE_RECOVER = 64    # rl_abi_features() bit 6: the recover stage
RL_RCV_MAX_NODES = 512
RCV_COLS = ("offset",)
RCV_SCAL = RTM_SCAL + ("lo0", "hi0")
RCV_INTS = RTM_INTS + ("clamped", "offtrack", "merge_node")
RCV_NODES = RTM_NODES + ("node_o", "node_k")


class RlRcvQuery(C.Structure):
    """``rl_rcv_query`` — the ``rl_rjn_query``, then merge_len [Q] and the optional dir_xy [Q][2]."""

    _fields_ = [("rj", RlRjnQuery), ("merge_len", C.POINTER(C.c_double)), ("dir_xy", C.POINTER(C.c_double))]


class RlRcv(C.Structure):
    """``rl_rcv`` — ``rl_rtm``'s layout, then offset [Q][M_cap], clamped, offtrack, merge_node, lo0,
    hi0 [Q] and the optional node_o, node_k [Q][K_cap + 1]; NULL fields are skipped."""

    _fields_ = (RlRtm._fields_ + [("offset", C.POINTER(C.c_double))] +
                [(n, C.POINTER(C.c_int32)) for n in RCV_INTS[len(RTM_INTS):]] +
                [(n, C.POINTER(C.c_double)) for n in RCV_SCAL[len(RTM_SCAL):] + RCV_NODES[len(RTM_NODES):]])


RL_FEATURE_FAN = 128       # rl_abi_features() bit 7: the fan stage
RL_FAN_MAX_CAND = 16
FAN_TAB_INTS = ("cand_class", "cand_feasible", "cand_clamped", "cand_merge_node", "cand_overspeed", "cand_bind_node")
FAN_TAB_SCAL = ("cand_t_end", "cand_t_loss", "cand_v_excess")


class RlFanQuery(C.Structure):
    """``rl_fan_query`` — the ``rl_rcv_query`` with merge_len [Q][n_cand], then n_cand."""

    _fields_ = [("rc", RlRcvQuery), ("n_cand", C.c_int32), ("_pad", C.c_int32)]


class RlFan(C.Structure):
    """``rl_fan`` — ``rl_rcv``'s layout holding the winner's values, then best [Q] and the table
    [Q][C]: class, feasible, clamped, merge_node, overspeed, bind_node, t_end, t_loss, v_excess of
    every candidate; NULL fields are skipped."""

    _fields_ = (RlRcv._fields_ + [("best", C.POINTER(C.c_int32))] +
                [(n, C.POINTER(C.c_int32)) for n in FAN_TAB_INTS] + [(n, C.POINTER(C.c_double)) for n in FAN_TAB_SCAL])


RL_FEATURE_BOUNDS = 16     # rl_abi_features() bit 4: the bounds stage
BND_ROWS = ("lo", "hi", "nx", "ny")
HZN_BND = ("lo", "hi", "lo0", "hi0")


class RlBndQuery(C.Structure):
    """``rl_bnd_query`` — the vehicle width and the safety margin of the guard, both finite."""

    _fields_ = [("veh_width", C.c_double), ("margin", C.c_double)]


class RlBnd(C.Structure):
    """``rl_bnd`` — caller-allocated lo, hi, nx, ny [R][N]; NULL fields are skipped."""

    _fields_ = [(n, C.POINTER(C.c_double)) for n in BND_ROWS]


class RlHznBnd(C.Structure):
    """``rl_hzn_bnd`` — caller-allocated lo, hi [Q][M_cap] and lo0, hi0 [Q]; NULL fields are skipped."""

    _fields_ = [(n, C.POINTER(C.c_double)) for n in HZN_BND]


RL_FEATURE_ROLLOUT = 256   # rl_abi_features() bit 8: the rollout stage
RL_RLL_MAX_ROLLOUTS = 65536
RL_RLL_MAX_STEPS = 512
RL_RLL_MAX_POSES = 1 << 22
RLL_POSE = ("u", "e", "dist2", "s", "margin", "vref")
RLL_INTS = ("count", "valid", "first_out")
RLL_SCAL = ("progress", "e_max", "margin_min", "cost")


class RlRllQuery(C.Structure):
    """``rl_rll_query`` — Q rollouts of T poses: xy [Q][T][2], the optional speeds v [Q][T], row and
    seg_hint [Q], the two windows, the four weights, hard_bounds, and group_size and k of the ranking."""

    _fields_ = [("xy", C.POINTER(C.c_double)), ("v", C.POINTER(C.c_double)), ("row", C.POINTER(C.c_int32)),
                ("seg_hint", C.POINTER(C.c_int32)), ("Q", C.c_int32), ("T", C.c_int32), ("window0", C.c_int32),
                ("window", C.c_int32), ("w_e", C.c_double), ("w_out", C.c_double), ("w_v", C.c_double),
                ("w_prog", C.c_double), ("hard_bounds", C.c_int32), ("group_size", C.c_int32), ("k", C.c_int32),
                ("_pad", C.c_int32)]


class RlRll(C.Structure):
    """``rl_rll`` — caller-allocated seg and u, e, dist2, s, margin, vref [Q][T], count, valid,
    first_out and progress, e_max, margin_min, cost [Q], order [G][k]; NULL fields are skipped."""

    _fields_ = ([("seg", C.POINTER(C.c_int32))] + [(n, C.POINTER(C.c_double)) for n in RLL_POSE] +
                [(n, C.POINTER(C.c_int32)) for n in RLL_INTS] + [(n, C.POINTER(C.c_double)) for n in RLL_SCAL] +
                [("order", C.POINTER(C.c_int32))])


OUT_F64 = ("x", "y", "heading", "kappa", "alpha_total", "alpha_last")
OUT_F64_MT = OUT_F64 + ("v", "ax")


def default_cfg() -> RlCfg:
    """cfg::Config defaults (main.cpp:77-113), computed in Python so the
    product path needs no oracle.  a_total_max = mu*9.81 (main.cpp:102)."""
    c = RlCfg()
    c.veh_width_m = 1.0
    c.safety_margin_m = 0.05
    c.lambda_smooth = 1.6e-3
    c.max_outer_iters = 14
    c.max_inner_iters = 120
    c.step_init = 0.65
    c.step_min = 1e-6
    c.armijo_c = 1e-5
    c.kappa_eps = 1e-6
    c.v_cap_mps = 27.0
    c.mass_kg = 255.0
    c.Cd = 0.30
    c.A_front_m2 = 1.00
    c.rho_air = 1.225
    c.c_rr = 0.015
    c.P_max_W = 80000.0
    c.mu = 1.17
    c.a_total_max = 1.17 * 9.81
    c.a_lat_max = 11.0
    c.a_long_acc_cap = 8.0
    c.a_long_brake_cap = 11.0
    c.w_time_gain = 1.0
    c.time_gamma_power = 2.0
    c.time_weight_use_inv_v = 0
    c.inv_v_gain = 0.1
    c.max_vpass_iters = 6
    c.use_total_ge_lat = 1
    return c


def set_mu(c: RlCfg, mu: float) -> None:
    """Sweep helper: a recompiled reference would evaluate a_total_max=mu*9.81 (main.cpp:102)."""
    c.mu = mu
    c.a_total_max = mu * 9.81


def dptr(a: Optional[np.ndarray]):
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_double))


def iptr(a: Optional[np.ndarray]):
    if a is None:
        return None
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_int32))


@dataclass
class Problem:
    """Inputs of compute_*_raceline (main.cpp:683-686): centerline [N,2], L,
    ring segments [E,4], veh_width (initial corridor only), closed."""

    center: np.ndarray
    L: float
    inner_seg: np.ndarray
    outer_seg: np.ndarray
    veh_width: float = 1.0
    closed: bool = True

    def __post_init__(self):
        self.center = np.ascontiguousarray(self.center, dtype=np.float64).reshape(-1, 2)
        self.inner_seg = np.ascontiguousarray(self.inner_seg, dtype=np.float64).reshape(-1, 4)
        self.outer_seg = np.ascontiguousarray(self.outer_seg, dtype=np.float64).reshape(-1, 4)

    @property
    def N(self) -> int:
        return int(self.center.shape[0])

    def as_c(self) -> RlProblem:
        p = RlProblem()
        p.center_xy = dptr(self.center)
        p.N = self.N
        p.closed = 1 if self.closed else 0
        p.L = float(self.L)
        p.inner_seg = dptr(self.inner_seg)
        p.Ei = int(self.inner_seg.shape[0])
        p.outer_seg = dptr(self.outer_seg)
        p.Eo = int(self.outer_seg.shape[0])
        p.veh_width = float(self.veh_width)
        return p


class HostPool:
    """Recycling allocator for the host result arrays of ``optimize_batch``.

    A caller of the drop-in that takes fresh arrays from every call and drops them after
    use makes the OS fault in ~100 MB of new pages per C2-sized call and unmap the old
    ones, and the next call's kernel runs slower behind that churn.  Arrays
    from this pool are views of a buffer the pool keeps mapped: when the last view of an
    array dies, its buffer returns to the pool (``weakref.finalize`` on the ctypes object
    the views are built on) and the next request of the same byte size gets it back, pages
    already resident.  An array is handed out again only after every view of it is gone, so
    results a caller keeps are never overwritten.  At most ``cap_bytes`` of free buffers
    are kept (``RL_HOST_POOL_MB``, default 1024; 0 disables the pool): a returned buffer
    that does not fit evicts the oldest free ones.  Arrays under ``min_bytes`` (256 KiB:
    malloc serves them from its heap, without mapping) are plain numpy arrays."""

    def __init__(self, cap_bytes: int, min_bytes: int = 1 << 18):
        self.cap = int(cap_bytes)
        self.min_bytes = int(min_bytes)
        self._free: list = []          # free uint8 buffers, oldest first
        self._free_bytes = 0
        self._lock = threading.Lock()
        self.hits = 0
        self.misses = 0

    def _release(self, buf: np.ndarray) -> None:
        # (a finalizer can run inside empty()'s locked region on this thread: never block)
        if buf.nbytes > self.cap or not self._lock.acquire(blocking=False):
            return
        try:
            while self._free and self._free_bytes + buf.nbytes > self.cap:
                self._free_bytes -= self._free.pop(0).nbytes
            self._free.append(buf)
            self._free_bytes += buf.nbytes
        finally:
            self._lock.release()

    def empty(self, shape, dtype) -> np.ndarray:
        """An uninitialised C-contiguous array, from a recycled buffer when one fits."""
        dt = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        if nbytes < self.min_bytes or nbytes > self.cap:
            return np.empty(shape, dtype=dt)
        buf = None
        with self._lock:
            for i in range(len(self._free) - 1, -1, -1):     # the most recently returned first
                if self._free[i].nbytes == nbytes:
                    buf = self._free.pop(i)
                    self._free_bytes -= nbytes
                    break
        if buf is None:
            self.misses += 1
            buf = np.empty(nbytes, dtype=np.uint8)
        else:
            self.hits += 1
        owner = (C.c_char * nbytes).from_buffer(buf)
        weakref.finalize(owner, self._release, buf).atexit = False
        return np.frombuffer(owner, dtype=dt).reshape(shape)

    def free_bytes(self) -> int:
        return self._free_bytes

    def clear(self) -> None:
        with self._lock:
            self._free.clear()
            self._free_bytes = 0


HOST_POOL = HostPool(int(float(os.environ.get("RL_HOST_POOL_MB", "1024")) * (1 << 20)))


@dataclass
class Outputs:
    """Host-side SoA result buffers [B][N] for one mode."""

    x: np.ndarray
    y: np.ndarray
    heading: np.ndarray
    kappa: np.ndarray
    alpha_total: np.ndarray
    alpha_last: np.ndarray
    evals: np.ndarray
    accepts: np.ndarray
    v: Optional[np.ndarray] = None
    ax: Optional[np.ndarray] = None
    lap: Optional[np.ndarray] = None
    vpass_sweeps: Optional[np.ndarray] = None

    @classmethod
    def alloc(cls, B: int, N: int, max_outer: int, mintime: bool, zero: bool = True,
              pool: Optional[HostPool] = None) -> "Outputs":
        """Result arrays of one mode; zero=False leaves them uninitialised (np.empty, or
        recycled buffers of ``pool``), for a call that writes every element (rl_optimize:
        every column, counter and lap)."""
        if zero:
            mk = np.zeros
        elif pool is not None:
            mk = pool.empty
        else:
            mk = np.empty
        z = lambda: mk((B, N), dtype=np.float64)  # noqa: E731
        o = cls(x=z(), y=z(), heading=z(), kappa=z(), alpha_total=z(), alpha_last=z(),
                evals=mk((B, max_outer), dtype=np.int32),
                accepts=mk((B, max_outer), dtype=np.int32))
        if mintime:
            o.v = z()
            o.ax = z()
            o.lap = mk(B, dtype=np.float64)
            o.vpass_sweeps = mk((B, max_outer + 1), dtype=np.int32)
        return o

    def as_c(self) -> RlOut:
        o = RlOut()
        for n in ("x", "y", "heading", "kappa", "alpha_total", "alpha_last", "v", "ax", "lap"):
            setattr(o, n, dptr(getattr(self, n)))
        o.evals = iptr(self.evals)
        o.accepts = iptr(self.accepts)
        o.vpass_sweeps = iptr(self.vpass_sweeps)
        return o


class RlSpline(C.Structure):
    """centerline::Spline1D (ref:403-446)."""
    _fields_ = [("s", C.POINTER(C.c_double)), ("a", C.POINTER(C.c_double)), ("b", C.POINTER(C.c_double)),
                ("c", C.POINTER(C.c_double)), ("d", C.POINTER(C.c_double)), ("n", C.c_int32), ("_pad", C.c_int32)]


class RlGeomProblem(C.Structure):
    """Inputs of pipeline::compute_geom_and_save (ref:1288-1335)."""
    _fields_ = [("spx", RlSpline), ("spy", RlSpline), ("s0", C.c_double), ("L", C.c_double),
                ("Kmax", C.c_int32), ("denomN", C.c_int32), ("emit_closed_duplicate", C.c_int32),
                ("closed", C.c_int32), ("inner_seg", C.POINTER(C.c_double)), ("outer_seg", C.POINTER(C.c_double)),
                ("Ei", C.c_int32), ("Eo", C.c_int32)]


RL_GEOM_COLS = 9
GEOM_COLS = ("s", "x", "y", "heading_rad", "curvature", "dist_to_inner", "dist_to_outer", "width", "v_kappa_mps")


@dataclass
class GeomProblem:
    """Step 6 inputs: the x(s), y(s) splines as knots [10][n] (x: s,a,b,c,d then y:
    s,a,b,c,d), s0, L, Kmax, denomN (ref:1308-1309), ring segments [E,4]."""

    knots: np.ndarray
    s0: float
    L: float
    Kmax: int
    denomN: int
    inner_seg: np.ndarray
    outer_seg: np.ndarray
    closed: bool = True
    emit_closed_duplicate: bool = True

    def __post_init__(self):
        self.knots = np.ascontiguousarray(self.knots, dtype=np.float64).reshape(10, -1)
        self.inner_seg = np.ascontiguousarray(self.inner_seg, dtype=np.float64).reshape(-1, 4)
        self.outer_seg = np.ascontiguousarray(self.outer_seg, dtype=np.float64).reshape(-1, 4)

    @property
    def rows(self) -> int:
        return int(self.Kmax) + (1 if self.emit_closed_duplicate else 0)

    def as_c(self) -> RlGeomProblem:
        g = RlGeomProblem()
        n = self.knots.shape[1]
        for sp, off in ((g.spx, 0), (g.spy, 5)):
            sp.s, sp.a, sp.b, sp.c, sp.d = (dptr(self.knots[off + j]) for j in range(5))
            sp.n = n
        g.s0, g.L = float(self.s0), float(self.L)
        g.Kmax, g.denomN = int(self.Kmax), int(self.denomN)
        g.emit_closed_duplicate = 1 if self.emit_closed_duplicate else 0
        g.closed = 1 if self.closed else 0
        g.inner_seg, g.outer_seg = dptr(self.inner_seg), dptr(self.outer_seg)
        g.Ei, g.Eo = self.inner_seg.shape[0], self.outer_seg.shape[0]
        return g


def cfg_array(cfgs) -> tuple:
    """list of RlCfg (or one) -> (ctypes array, n)."""
    if isinstance(cfgs, RlCfg):
        cfgs = [cfgs]
    arr = (RlCfg * len(cfgs))(*cfgs)
    return arr, len(cfgs)


def seed_array(seeds) -> Optional[np.ndarray]:
    if seeds is None:
        return None
    return np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))


def u64ptr(a: Optional[np.ndarray]):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


_P = C.POINTER
_PROB, _CFG, _OUT, _SEL = _P(RlProblem), _P(RlCfg), _P(RlOut), _P(RlSelect)
_F64, _F32, _I32, _I64, _U64 = _P(C.c_double), _P(C.c_float), _P(C.c_int32), _P(C.c_int64), _P(C.c_uint64)
_BATCH = [_PROB, _CFG, C.c_int32, _U64, C.c_int32]       # problem, cfgs, ncfg, seeds, B
_BEST = [_I32, _F64, _F64, _OUT]                          # index, score, scores, the winners' rows

# every function of rl_abi.h (ABI 6.1): (name, restype, argtypes); argtypes None = not declared
DECLS = [
    ("rl_optimize", C.c_int, _BATCH + [_OUT, _OUT]),
    ("rl_cfg_default", None, [_CFG]),
    ("rl_cfg_set_mu", None, [_CFG, C.c_double]),
    ("rl_ring_segments", C.c_int, [_F64, C.c_int32, C.c_int32, _F64]),
    ("rl_seed_value", C.c_double, [C.c_uint64, C.c_int32, C.c_double]),
    ("rl_plan_create", C.c_int, [_P(C.c_void_p), C.c_int32] + _BATCH + [C.c_int32]),
    ("rl_plan_run", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rl_plan_run_group", C.c_int, [_P(C.c_void_p), C.c_int32, C.c_void_p]),
    ("rl_plan_fetch", C.c_int, [C.c_void_p, _OUT, _OUT]),
    ("rl_plan_device_outputs", C.c_int, [C.c_void_p, C.c_int32, _OUT]),
    ("rl_plan_bind_device_outputs", C.c_int, [C.c_void_p, C.c_int32, _OUT]),
    ("rl_plan_kernel_ms", C.c_int, [C.c_void_p, C.c_int32, _F32]),
    ("rl_plan_destroy", C.c_int, [C.c_void_p]),
    ("rl_plan_set_shape_batch", C.c_int, [C.c_void_p, C.c_int32]),
    ("rl_plan_shape", C.c_int, [C.c_void_p, C.c_int32, _I32, _I32]),
    ("rl_device_count", C.c_int, None),
    ("rl_last_error", C.c_char_p, None),
    ("rl_abi_version", C.c_int, None),
    ("rl_abi_minor", C.c_int, None),
    ("rl_kernel_variant", C.c_int, [C.c_int32]),
    ("rl_kernel_shape", C.c_int, [C.c_int32, C.c_int32, C.c_int32, _I32, _I32]),
    ("rl_geom", C.c_int, [_P(RlGeomProblem), _CFG, C.c_int32, _F64, _F32]),
    ("rl_corridor", C.c_int, [_PROB, _CFG, C.c_int32, _F64, _F64]),
    ("rl_lap_eval", C.c_int, [_F64, _F64, C.c_int32, C.c_int32, C.c_int32, _CFG, C.c_int32, C.c_int32, _OUT, _F32]),
    ("rl_format_csv", C.c_int, [_F64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, _I64, _I64]),
    ("rl_optimize_multi", C.c_int, _BATCH + [_I32, C.c_int32, _OUT, _OUT]),
    ("rl_last_call_ms", C.c_int, [_F32, _F32]),
    ("rl_release_plan_cache", C.c_int, []),
    ("rl_last_call_times", C.c_int, [_F32] * 4),
    ("rl_plan_cache_info", C.c_int, [_I32, _I64, _I64]),
    ("rl_last_call_download", C.c_int, [_I32, _I32]),
    ("rl_plan_select", C.c_int, [C.c_void_p, _SEL, C.c_void_p]),
    ("rl_plan_fetch_selected", C.c_int, [C.c_void_p] + _BEST),
    ("rl_optimize_best", C.c_int, _BATCH + [_SEL] + _BEST),
    ("rl_rank_scores", C.c_int, [_F64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _I32]),
    ("rl_plan_lap", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rl_plan_fetch_lap", C.c_int, [C.c_void_p, _OUT, _F64]),
    ("rl_plan_select_scored", C.c_int, [C.c_void_p, _SEL, C.c_int32, C.c_void_p]),
    ("rl_optimize_best_scored", C.c_int, _BATCH + [_SEL, C.c_int32] + _BEST),
    ("rl_path_lengths", C.c_int, [_F64, _F64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F64]),
]

# additions that leave RL_ABI_MINOR as it is (rl_abi_features() names them); bound like DECLS
_TRAJ = _P(RlTraj)
DECLS_EXT = [
    ("rl_abi_features", C.c_int, []),
    ("rl_plan_trajectory", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_void_p]),
    ("rl_plan_fetch_trajectory", C.c_int, [C.c_void_p, _TRAJ]),
    ("rl_optimize_best_trajectory", C.c_int, _BATCH + [_SEL, C.c_int32] + _BEST + [C.c_double, C.c_int32, _TRAJ]),
    ("rl_trajectory", C.c_int, [_F64] * 7 + [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, _TRAJ]),
]

# The pose-query stages, one row each: name (rl_plan_<name>, rl_plan_fetch_<name>, rl_<name>), feature
# bit, query struct, results struct, and the row arguments of the one-shot (x, y, heading, kappa, v,
# ax, h; with lo, hi, nx, ny for a stage that reads the bounds: 11).  A stage is bound only in a
# library whose rl_abi_features() has its bit.
QUERY_STAGES = (
    ("horizon", RL_FEATURE_HORIZON, RlHznQuery, RlHzn, 7),
    ("rejoin", RL_FEATURE_REJOIN, RlRjnQuery, RlRjn, 7),
    ("stop", RL_FEATURE_STOP, RlStpQuery, RlStp, 7),
    ("retime", RL_FEATURE_RETIME, RlRtmQuery, RlRtm, 7),
    ("recover", RL_FEATURE_RECOVER, RlRcvQuery, RlRcv, 11),
    ("recover_fan", RL_FEATURE_FAN, RlFanQuery, RlFan, 11),
)


def _stage_decls(name, _feature, query, results, n_rows) -> list:
    return [("rl_plan_" + name, C.c_int, [C.c_void_p, _P(query), C.c_void_p]),
            ("rl_plan_fetch_" + name, C.c_int, [C.c_void_p, _P(results)]),
            ("rl_" + name, C.c_int, [_F64] * n_rows + [C.c_int32, C.c_int32, C.c_int32, _P(query), C.c_int32, _P(results)])]


DECLS_HZN, DECLS_RJN, DECLS_STP, DECLS_RTM, DECLS_RCV, DECLS_FAN = (_stage_decls(*st) for st in QUERY_STAGES)

# the bounds stage: bound only in a library whose rl_abi_features() has RL_FEATURE_BOUNDS
_BND, _BNDQ, _HZNBND = _P(RlBnd), _P(RlBndQuery), _P(RlHznBnd)
DECLS_BND = [
    ("rl_plan_bounds", C.c_int, [C.c_void_p, _BNDQ, C.c_void_p]),
    ("rl_plan_fetch_bounds", C.c_int, [C.c_void_p, _BND]),
    ("rl_plan_horizon_bounds", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rl_plan_fetch_horizon_bounds", C.c_int, [C.c_void_p, _HZNBND]),
    ("rl_bounds", C.c_int, [_P(RlProblem), _F64, _F64, C.c_int32, C.c_double, C.c_double, C.c_int32, _BND]),
]


# the rollout stage: bound only in a library whose rl_abi_features() has RL_FEATURE_ROLLOUT
_RLL, _RLLQ = _P(RlRll), _P(RlRllQuery)
DECLS_RLL = [
    ("rl_plan_rollouts", C.c_int, [C.c_void_p, _RLLQ, C.c_void_p]),
    ("rl_plan_fetch_rollouts", C.c_int, [C.c_void_p, _RLL]),
    ("rl_rollouts", C.c_int, [_F64] * 9 + [C.c_int32, C.c_int32, C.c_int32, _RLLQ, C.c_int32, _RLL]),
]


def declare_optimize(fn) -> None:
    """rl_optimize's signature (the oracle's oracle_optimize shares it)."""
    fn.restype, fn.argtypes = DECLS[0][1], DECLS[0][2]


_LIB = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Load librl.so (the HIP path).  Raises if it is missing: there is no fallback; a library
    that lacks a function of DECLS or DECLS_EXT raises AttributeError naming it, and so does
    one that announces RL_FEATURE_HORIZON / RL_FEATURE_REJOIN / RL_FEATURE_STOP /
    RL_FEATURE_BOUNDS / RL_FEATURE_RETIME / RL_FEATURE_RECOVER / RL_FEATURE_FAN / RL_FEATURE_ROLLOUT and
    lacks a function of DECLS_HZN / DECLS_RJN / DECLS_STP / DECLS_BND / DECLS_RTM / DECLS_RCV / DECLS_FAN /
    DECLS_RLL."""
    global _LIB
    if _LIB is not None and path == LIB_PATH:
        return _LIB
    if not os.path.exists(path):
        raise RuntimeError(f"librl.so not built at {path}: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(path)
    # a library built from an earlier revision (RL_LIB: A/B against a parent) has no
    # rl_abi_features and none of DECLS_EXT; one that has it must have them all
    ext = DECLS_EXT if hasattr(lib, "rl_abi_features") else []
    def bind(decls):
        for name, restype, argtypes in decls:
            fn = getattr(lib, name)
            fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes

    bind(DECLS + ext)
    features = lib.rl_abi_features() if ext else 0
    for st in QUERY_STAGES:
        if features & st[1]:
            bind(_stage_decls(*st))
    if features & RL_FEATURE_BOUNDS:
        bind(DECLS_BND)
    if features & RL_FEATURE_ROLLOUT:
        bind(DECLS_RLL)
    if path == LIB_PATH:
        _LIB = lib
    return lib


def kernel_shape(N: int, B: int, mode: int) -> tuple:
    """(K samples per lane, T lanes per instance) librl.so launches for (N, B, mode)."""
    lib = load_library()
    k, t = C.c_int32(), C.c_int32()
    rc = lib.rl_kernel_shape(int(N), int(B), int(mode), C.byref(k), C.byref(t))
    if rc != RL_OK:
        raise RuntimeError(f"rl_kernel_shape({N}, {B}, {mode}) = {rc}")
    return k.value, t.value


def cfg_field_names() -> list:
    return [n for n, _ in RlCfg._fields_ if not n.startswith("_")]


__all__ = [n for n in dir() if not n.startswith("_") and n not in ("C", "os", "np", "fields", "dataclass", "Optional")]
