"""An exact-arithmetic reference of the time-domain resampling family: the trajectory stage
(rl_trajectory.hip), the horizon stage (rl_horizon.hip and the device functions of rl_horizon.h)
and the tick kernel of rl_bounds.hip.  A plain helper module like oracle_lib and query_cases: no
fixtures, no pytest settings.

The operations are stated here from the words of DESIGN 3k, 3l and 3o in rational arithmetic
(fractions.Fraction; every double converts exactly) with linear scans only.  Nothing is shared
with raceline.py: no searchsorted, no bisection, none of its helpers.  What a stage returns
(raceline.trajectory_host or raceline.trajectory, horizon_host or horizon, horizon_bounds_host or
a plan's horizon_bounds) is checked against these statements within bounds that follow from
counting the roundings of DESIGN's formulas; each derivation stands in the docstring of the
helper that applies it.  Throughout EPS = 2**-53, the unit roundoff: one operation returns its
exact result times (1 + d), |d| <= EPS.  Terms of order EPS**2 are covered by the room between
the counted roundings and the constants 8, 64 and 4.

Every tick and every query of a result is checked.  Three checks are skipped where their answer
is not defined by the data: the sign of e when the exact cross product is within its own rounding
of 0 ("cross"), the choice of arc when two headings are half a turn apart ("arc"), and the count
of an open row when a tick lies within its own rounding of T ("count").  A Tally counts how often
each applied and to how many items; the tests assert on it.
"""
import math
from fractions import Fraction as F

import numpy as np

EPS = F(1, 2 ** 53)
PI = F(math.pi)                         # M_PI, the kernels' pi, exactly
TWO_PI = 2 * PI
ARC_NEAR = F(1, 2 ** 50)
LERP_COLS = ("x", "y", "kappa", "v")    # a_i + u (a_j - a_i)


class Tally:
    """How many items each of the three skips could have applied to, and on how many it fired."""

    KINDS = ("cross", "arc", "count")

    def __init__(self):
        self.items = dict.fromkeys(self.KINDS, 0)
        self.fired = dict.fromkeys(self.KINDS, 0)
        self.ticks = 0                  # horizon ticks checked
        self.multi = 0                  # of which with more than one admissible segment
        self.worst = {}                 # label -> the largest error / bound seen

    def add(self, kind, fired):
        self.items[kind] += 1
        self.fired[kind] += bool(fired)

    def ratio(self, label, err, bound):
        if bound > 0:
            self.worst[label] = max(self.worst.get(label, 0.0), float(err / bound))

    def share(self, kind):
        return self.fired[kind] / self.items[kind] if self.items[kind] else 0.0

    def assert_skips_rare(self, label=""):
        """Each skip fired on fewer than 5 % of the items it could apply to."""
        for k in self.KINDS:
            assert self.share(k) < 0.05, f"{label}: skip '{k}' fired on {self.fired[k]} of {self.items[k]} items"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return bits([a])[0] == bits([b])[0]


# ---------------------------------------------------------------------------- stamps and counts
def exact_stamps(v, h):
    """The stamps t[0..N] of one row: t_0 = 0, t_{i+1} = float(Fraction(t_i) + Fraction(inc_i)),
    inc_i = float(Fraction(h) / Fraction(max(1e-6, v_i))).  Fraction.__float__ rounds correctly,
    so each step is the IEEE quotient and the IEEE sum: this is the serial sum in index order,
    bit for bit, and nothing else is.  A v that is not above 1e-6 (a NaN too) counts as 1e-6; an
    infinite v gives the increment 0, the IEEE quotient."""
    t = [0.0]
    h = float(h)
    for vi in np.asarray(v, dtype=np.float64).tolist():
        vv = vi if 1e-6 < vi else 1e-6
        inc = 0.0 if math.isinf(vv) else float(F(h) / F(vv))
        t.append(float(F(t[-1]) + F(inc)))
    return t


def tick_count(T, dt, m_cap):
    """min(m_cap, #{m : float(m) * dt < T}) by a linear scan in Python floats (m -> float(m) * dt
    does not decrease, so the scan may stop at the first failure); 0 when T is not finite."""
    if not math.isfinite(T):
        return 0
    m = 0
    while m < m_cap and float(m) * dt < T:
        m += 1
    return m


def check_stamps(stamps_row, T, v, h, S, label=""):
    """stamps bit-equal to exact_stamps, T bit-equal to stamps[S]."""
    want = exact_stamps(v, h)
    got = np.asarray(stamps_row, dtype=np.float64)
    assert got.shape == (len(want),), f"{label}: stamps shape {got.shape}"
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert bad.size == 0, f"{label}: stamp {bad[0]} is {got[bad[0]]!r}, the serial sum gives {want[bad[0]]!r}"
    assert same_bits(T, want[S]), f"{label}: T {T!r} != stamps[S] {want[S]!r}"
    return want


# ---------------------------------------------------------------------------- the columns
def _lerp_check(tally, name, got, ai, aj, u, slack, mag=None):
    """got against a_i + u (a_j - a_i), u exact.  The kernel computes
    fl(a_i + fl(u^ * fl(a_j - a_i))) with u^ = fl(fl(tau - t_i) / fl(t_{i+1} - t_i)): three
    roundings in u^ (two differences, one quotient), one in the difference, one in the product,
    so the product is u (a_j - a_i) (1 + 5 EPS) with |u (a_j - a_i)| <= |a_i| + |a_j|, and one
    in the sum, whose result is at most |a_i| + |a_j| too: 6 EPS (|a_i| + |a_j|), bounded by
    8 EPS (|a_i| + |a_j|).  slack adds what the caller knows about u (the horizon's L * delta).
    An end that is not finite (v = inf on a stretch) has no exact value: IEEE arithmetic then
    gives an infinity or a NaN for every u, and that is what is asked."""
    if not (math.isfinite(ai) and math.isfinite(aj)):
        return None if not math.isfinite(got) else f"{name}: {got!r} between {ai!r} and {aj!r}"
    if not math.isfinite(got):
        return f"{name}: {got!r} between {ai!r} and {aj!r}"
    exact = F(ai) + u * (F(aj) - F(ai))
    room = 8 * EPS * (abs(F(ai)) + abs(F(aj))) if mag is None else mag
    err = abs(F(got) - exact)
    if err <= room + slack:
        tally.ratio(name, err, room + slack)
        return None
    return f"{name}: {got!r}, exact {float(exact)!r}, off by {float(err):.3e} > {float(room + slack):.3e}"


def _arcs(pi_, pj):
    """The admissible differences psi_j - psi_i: the shorter arc, d less 2 pi if d > pi, plus 2 pi
    if d < -pi (pi = M_PI); both arcs when ||d| - pi| <= 2**-50, since the kernel decides with a
    rounded d, off by at most EPS (|psi_i| + |psi_j|)."""
    d = F(pj) - F(pi_)
    short = d - TWO_PI if d > PI else d + TWO_PI if d < -PI else d
    if abs(abs(d) - PI) <= ARC_NEAR:
        return [short, short - TWO_PI if short > 0 else short + TWO_PI], True
    return [short], False


def _heading_check(tally, got, pi_, pj, u, slack):
    """got against psi_i + u d modulo 2 pi, d the shorter arc.  Roundings: one in psi_j - psi_i,
    one more (of a value below 2 pi, with M_PI's own 2**-53 relative distance from pi) when 2 pi
    is added or taken, three in u^, one in the product, one in the sum: 7 EPS of at most
    |psi_i| + |psi_j| + 2 pi, bounded by 8 EPS (|psi_i| + |psi_j| + 2 pi).  slack is the
    horizon's L * delta."""
    arcs, near = _arcs(pi_, pj)
    tally.add("arc", near)
    if not math.isfinite(got):
        return f"heading: {got!r}"
    room = 8 * EPS * (abs(F(pi_)) + abs(F(pj)) + TWO_PI)
    best = None
    for d in arcs:
        diff = F(got) - (F(pi_) + u * d)
        r = abs(diff - round(diff / TWO_PI) * TWO_PI)
        bound = room + slack
        if r <= bound:
            tally.ratio("heading", r, bound)
            return None
        best = r if best is None else min(best, r)
    return f"heading: {got!r} is {float(best):.3e} from the shorter arc modulo 2 pi, allowed {float(room):.3e}"


def _s_check(tally, got, lap, S, i, u, h, slack):
    """got against (lap S + i + u) h.  lap * S + i is exact in doubles; adding u^ (three
    roundings, u^ <= 1) rounds a sum of at most lap S + i + 1, and the product with h rounds
    once more: 3 EPS u h + 2 EPS (lap S + i + 1) h, bounded by 8 EPS (lap S + i + 1) h."""
    exact = (lap * S + i + u) * F(h)
    room = 8 * EPS * (lap * S + i + 1) * abs(F(h))
    err = abs(F(got) - exact) if math.isfinite(got) else None
    if err is not None and err <= room + slack:
        tally.ratio("s", err, room + slack)
        return None
    return f"s: {got!r}, exact {float(exact)!r}, allowed {float(room + slack):.3e}"


# ---------------------------------------------------------------------------- the trajectory stage
def check_trajectory(traj, rows, h, closed, dt, m_cap, tally, source=None, label=""):
    """Every row of a Trajectory against the rows it was made from (rows: x, y, heading, kappa, v,
    ax [B, N]; h [B] or a number; source[r]: the row of output row r, None: r).  Stamps, T and
    count as above; tick m at tau = float(m) * dt lies on the one segment i with
    t_i <= tau < t_{i+1}, found by a linear scan (asserted unique); u* = (tau - t_i) /
    (t_{i+1} - t_i) exactly, j = (i + 1) mod N; x, y, kappa, v by _lerp_check, s by _s_check,
    heading by _heading_check, ax bit-equal to ax_i."""
    X, Y, PSI, K, V, A = (np.asarray(a, dtype=np.float64) for a in rows)
    Bn, N = X.shape
    hs = np.broadcast_to(np.asarray(h, dtype=np.float64), (Bn,))
    S = N if closed else N - 1
    R = len(traj.count)
    checked = 0
    for r in range(R):
        b = r if source is None else int(source[r])
        lab = f"{label} row {r}"
        t = check_stamps(traj.stamps[r], traj.T[r], V[b], hs[b], max(S, 0), lab)
        count = tick_count(t[max(S, 0)], dt, m_cap) if S > 0 else 0
        assert int(traj.count[r]) == count, f"{lab}: count {traj.count[r]}, the scan gives {count}"
        ta = np.array(t[:S + 1])
        for m in range(count):
            tau = float(m) * dt
            hit = np.nonzero((ta[:-1] <= tau) & (tau < ta[1:]))[0]
            assert hit.size == 1, f"{lab} tick {m}: {hit.size} segments hold tau"
            i = int(hit[0])
            j = (i + 1) % N
            u = (F(tau) - F(t[i])) / (F(t[i + 1]) - F(t[i]))
            errs = [_lerp_check(tally, n, float(getattr(traj, n)[r, m]), float(a[b, i]), float(a[b, j]), u, 0)
                    for n, a in zip(LERP_COLS, (X, Y, K, V))]
            errs.append(_s_check(tally, float(traj.s[r, m]), 0, S, i, u, hs[b], 0))
            errs.append(_heading_check(tally, float(traj.heading[r, m]), float(PSI[b, i]), float(PSI[b, j]), u, 0))
            if not same_bits(traj.ax[r, m], A[b, i]):
                errs.append(f"ax: {traj.ax[r, m]!r}, segment {i} has {A[b, i]!r}")
            errs = [e for e in errs if e]
            assert not errs, f"{lab} tick {m} (segment {i}): " + "; ".join(errs)
            checked += 1
    return checked


# ---------------------------------------------------------------------------- the locate
def candidates(S, g, W, closed):
    """DESIGN 3l's candidates as a set: every i in [0, S) without a hint (g = -1); on a closed
    row (g + k) mod S for k = -W .. W, all of [0, S) if 2 W + 1 >= S; on an open row
    max(0, g - W) .. min(S - 1, g + W)."""
    if S < 1:
        return set()
    if g < 0:
        return set(range(S))
    if closed:
        return set(range(S)) if 2 * W + 1 >= S else {(g + k) % S for k in range(-W, W + 1)}
    return set(range(max(0, g - W), min(S - 1, g + W) + 1))


def exact_foot(xi, yi, xj, yj, px, py):
    """The clamped foot of p on the segment from (xi, yi) to (xj, yj), exactly: u* = c / dd clamped
    to [0, 1] (0 on a zero-length segment), D* = |w - u* d|^2, and what the bounds need."""
    dx, dy, wx, wy = F(xj) - F(xi), F(yj) - F(yi), F(px) - F(xi), F(py) - F(yi)
    dd, ww = dx * dx + dy * dy, wx * wx + wy * wy
    u = F(0) if dd == 0 else min(F(1), max(F(0), (wx * dx + wy * dy) / dd))
    rx, ry = wx - u * dx, wy - u * dy
    return dict(u=u, D=rx * rx + ry * ry, m=abs(wx) + abs(wy) + abs(dx) + abs(dy), dd=dd, ww=ww,
                cross=dx * wy - dy * wx, on_end=dd == 0 or ww == 0 or (wx, wy) == (dx, dy))


def _near_candidates(X, Y, N, cand, px, py):
    """The candidates that can hold the least D*, by a linear pass in doubles.  Every point of
    segment i is within |d_i| / 2 of its midpoint, so D*_i >= (|p - mid_i| - |d_i| / 2)^2, and
    D*_i <= |p - x_i|^2.  A candidate whose lower bound exceeds the least upper bound by more than
    a margin (1e-9 of the coordinates' size, some 1e6 roundings) cannot be a minimiser and is
    left out of the exact pass; nothing else is."""
    c = np.array(sorted(cand), dtype=np.int64)
    j = (c + 1) % N
    mx, my = 0.5 * (X[c] + X[j]), 0.5 * (Y[c] + Y[j])
    half = 0.5 * np.hypot(X[j] - X[c], Y[j] - Y[c])
    lb = np.maximum(0.0, np.hypot(px - mx, py - my) - half)
    ub = np.hypot(px - X[c], py - Y[c])
    scale = 1.0 + max(abs(px), abs(py), float(np.max(np.abs(X))), float(np.max(np.abs(Y))))
    return [int(i) for i in c[lb <= np.min(ub) + 1e-9 * scale]]


def _sqrt_up(q):
    """A Fraction not below sqrt(q), and within 2**-50 of it relatively."""
    return F(math.sqrt(float(q))) * (1 + F(1, 2 ** 50))


def check_locate(hz, rows, stamps, h, closed, poses, row, hint, W, tally, feet=None, label=""):
    """seg, u, dist2, e, t0, s0 and (for poses without a segment) count of every query.

    With w = p - x_i, d = x_j - x_i exact and m = |wx| + |wy| + |dx| + |dy|, the kernel's
    roundings: each of wx, wy, dx, dy once.  dd^ = dd (1 + 4 EPS) (inputs twice, product, sum).
    c^ = c +- 4 EPS (|wx dx| + |wy dy|) <= c +- 4 EPS |w| |d| (Cauchy-Schwarz), an absolute
    error since the two products may cancel.  The quotient rounds once more, and the clamp to
    [0, 1] does not widen a distance, so |u^ - u*| <= 5 EPS + 4 EPS |w| / |d|, bounded by
    8 EPS (1 + |w| / |d|).  On a zero-length segment u^ = u* = 0.
    rx^ = fl(wx^ - fl(u^ dx^)): EPS |wx| from wx^, |u^ - u*| |dx| + 2 EPS |dx| from the product
    and EPS (|wx| + |dx|) from the difference, at most 8 EPS m with |w| <= |wx| + |wy|; the same
    for ry^.  D^ = fl(rx^ rx^ + ry^ ry^) = D* + 2 (rx drx + ry dry) + 3 EPS D*, and
    |rx| + |ry| <= m, D* <= m^2: |D^ - D*| <= 16 EPS m^2 + 3 EPS m^2 <= 32 EPS m^2.
    The winner has the least computed D^, so D*(seg) <= D*(i) + 32 EPS (m_seg^2 + m_i^2) for the
    exact minimiser i: D*(seg) <= min D* + 64 EPS max(m_seg, m_i)^2, and dist2 = D^(seg) lies
    within 32 EPS m_seg^2, inside the same bound, of D*(seg).
    |e| is sqrt(dist2), correctly rounded.  The cross product dx wy - dy wx is computed within
    4 EPS (|dx wy| + |dy wx|) <= 4 EPS |d| |w|; its sign is asked unless |cross| <= 8 EPS |d| |w|.
    Where d = 0, w = 0 or w = d in doubles (a zero-length segment, a pose exactly on an end) the
    computed cross product is a zero whatever the roundings, so e is not negative: no skip.
    t0 = fl(t_i + fl(u^ fl(t_{i+1} - t_i))): three roundings of values up to t_{i+1}, and
    |u^ - u*| (t_{i+1} - t_i) from u^; s0 = fl(fl(i + u^) h): two roundings of values up to
    (i + 1) h, and |u^ - u*| h.  With the 5 EPS + 4 EPS |w| / |d| above both stay inside
    8 EPS t_{i+1} and 8 EPS (i + 1) h whenever the u term is at most 5 EPS of the magnitude, that
    is for a clamped foot (u^ = u* in {0, 1} unless the foot is within the rounding of an end)
    and for any foot once (1 + |w| / |d|) (t_{i+1} - t_i) <= t_{i+1}; a far pose on the first
    segments is always clamped.
    A pose exactly on a sample has D* = D^ = 0 on every candidate that ends there (w = 0 gives
    u^ = 0, w = d gives c^ = dd^ and u^ = 1, r^ = 0): the least such candidate must win.
    A NaN pose or an empty candidate set: seg = -1 and count = 0.
    feet caches exact_foot per (row, query, segment) across calls with the same poses."""
    X, Y = (np.asarray(a, dtype=np.float64) for a in rows[:2])
    Bn, N = X.shape
    hs = np.broadcast_to(np.asarray(h, dtype=np.float64), (Bn,))
    S = N if closed else N - 1
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 2)
    Q = P.shape[0]
    row = np.zeros(Q, dtype=np.int64) if row is None else np.asarray(row)
    hint = np.full(Q, -1) if hint is None else np.broadcast_to(np.asarray(hint), (Q,))
    feet = {} if feet is None else feet
    assert len(hz.seg) == Q
    for q in range(Q):
        b, px, py = int(row[q]), float(P[q, 0]), float(P[q, 1])
        lab = f"{label} query {q}"
        cand = candidates(S, int(hint[q]), int(W), closed)
        seg = int(hz.seg[q])
        if not cand or math.isnan(px) or math.isnan(py):
            assert seg == -1 and int(hz.count[q]) == 0, f"{lab}: seg {seg}, count {hz.count[q]} for no candidate or a NaN pose"
            continue
        assert seg in cand, f"{lab}: seg {seg} is no candidate"

        def foot(i):
            key = (b, q, i)
            if key not in feet:
                j = (i + 1) % N
                feet[key] = exact_foot(X[b, i], Y[b, i], X[b, j], Y[b, j], px, py)
            return feet[key]

        near = _near_candidates(X[b], Y[b], N, cand, px, py)
        best = min(near, key=lambda i: (foot(i)["D"], i))
        fs, fb = foot(seg), foot(best)
        room = 64 * EPS * max(fs["m"], fb["m"]) ** 2
        excess = fs["D"] - fb["D"]
        assert excess <= room, (f"{lab}: seg {seg} at D* {float(fs['D'])!r}, segment {best} at {float(fb['D'])!r}: "
                                f"excess {float(excess):.3e} > {float(room):.3e}")
        tally.ratio("locate excess", max(excess, 0), room)
        zero = [i for i in near if foot(i)["D"] == 0]
        on_sample = any((px, py) == (float(X[b, k]), float(Y[b, k])) for i in zero for k in (i, (i + 1) % N))
        if zero and on_sample:
            assert seg == min(zero), f"{lab}: on a sample, candidates {zero} at distance 0, seg {seg}"
        d2 = float(hz.dist2[q])
        assert math.isfinite(d2) and d2 >= 0.0, f"{lab}: dist2 {d2!r}"
        err = abs(F(d2) - fs["D"])
        assert err <= room, f"{lab}: dist2 {d2!r}, D* {float(fs['D'])!r}, off by {float(err):.3e} > {float(room):.3e}"
        tally.ratio("dist2", err, room)
        u = float(hz.u[q])
        if fs["dd"] == 0:
            assert u == 0.0, f"{lab}: u {u!r} on a zero-length segment"
        else:
            uroom = 8 * EPS * (1 + _sqrt_up(fs["ww"] / fs["dd"]))
            err = abs(F(u) - fs["u"])
            assert err <= uroom, f"{lab}: u {u!r}, u* {float(fs['u'])!r}, off by {float(err):.3e} > {float(uroom):.3e}"
            tally.ratio("u", err, uroom)
        e = float(hz.e[q])
        assert same_bits(abs(e), math.sqrt(d2)), f"{lab}: |e| {abs(e)!r} != sqrt(dist2) {math.sqrt(d2)!r}"
        flat = not fs["on_end"] and fs["cross"] ** 2 <= (8 * EPS) ** 2 * fs["dd"] * fs["ww"]
        tally.add("cross", flat)
        if not flat:
            assert (math.copysign(1.0, e) < 0.0) == (fs["cross"] < 0), f"{lab}: e {e!r}, exact cross product {float(fs['cross'])!r}"
        t = stamps[b]
        ti, tj = F(float(t[seg])), F(float(t[seg + 1]))
        t0 = float(hz.t0[q])
        err = abs(F(t0) - (ti + fs["u"] * (tj - ti)))
        assert err <= 8 * EPS * tj, f"{lab}: t0 {t0!r} off by {float(err):.3e} > {float(8 * EPS * tj):.3e}"
        tally.ratio("t0", err, 8 * EPS * tj)
        bad = _s_check(tally, float(hz.s0[q]), 0, S, seg, fs["u"], hs[b], 0)
        assert not bad, f"{lab}: s0: {bad}"
    return feet


# ---------------------------------------------------------------------------- the horizon's ticks
def _admissible(t, S, T, tau, delta, closed):
    """The (lap, segment) pairs a tick at tau* may lie on: c* = floor(tau* / T) and
    w* = tau* - c* T on a closed row, c* = 0 and w* = tau* on an open one; the segments of positive
    duration whose [t_i, t_{i+1}) widened by delta holds w*, and around the start line those that
    hold w* + T in lap c* - 1 or w* - T in lap c* + 1.  The kernel's w^ satisfies
    t_i <= w^ < t_{i+1} and |w^ - w*| <= delta, so t_i - delta <= w* < t_{i+1} + delta: the upper
    end stays open, and with delta = 0 this is DESIGN's own rule.  A linear pass in doubles with a margin of
    twice delta and 2**-40 of the time picks the segments the exact comparison is made on."""
    laps = [0]
    if closed:
        c = math.floor(tau / T)
        laps = [k for k in (c - 1, c, c + 1) if k >= 0]
    out = []
    for k in laps:
        w = tau - k * T
        wf = float(w)
        mar = 2.0 * float(delta) + abs(wf) * 2.0 ** -40 + 5e-324
        for i in np.nonzero((t[:S] <= wf + mar) & (t[1:S + 1] >= wf - mar) & (t[1:S + 1] > t[:S]))[0]:
            if F(float(t[i])) - delta <= w < F(float(t[i + 1])) + delta:
                out.append((k, int(i), w))
    return out


def check_horizon_ticks(hz, rows, stamps, h, closed, row, dt, m_cap, tally, label=""):
    """count and every tick of every located query, from the stage's own t0.

    tau* = t0 + m dt exactly.  The kernel has tau^ = fl(t0 + fl(m dt)), within 2 EPS tau* of it.
    Closed rows: c^ = floor(fl(tau^ / T)), w^ = fl(tau^ - fl(c^ T)) and at most one fix-up each
    way, so c^ T + w^ is tau^ but for the rounding of the product (EPS c^ T <= EPS tau*) and of
    the difference (EPS w^ <= EPS tau*): the kernel's row time is within delta = 4 EPS tau* of
    tau* - c^ T, where c^ is c* or, for a tick within delta of the start line, its neighbour.
    Open rows: c^ = 0, w^ = tau^.  Tick 0 is exact, delta = 0: tau^ = t0 + 0 is t0 itself, at most T,
    so c^ is 0 or 1, c^ T is exact and so is the difference.  So the tick's segment is one of _admissible's, and its u is
    (w - t_i) / (t_{i+1} - t_i) within delta / (t_{i+1} - t_i) and the three roundings of u^.
    Each column then lies within L delta + 8 EPS (magnitude) of the segment's own line at w, L
    the greatest slope |a_j - a_i| / (t_{i+1} - t_i) over the admissible segments (for s the
    slope h / (t_{i+1} - t_i) and the magnitude (c S + i + 1) h; for the heading the arc's
    slope); ax is bit-equal to ax_i.  A tick passes when one admissible (lap, segment) explains
    all seven columns.  count: closed rows m_cap when T is finite and positive, else 0; open
    rows #{tau* < T}, give or take the tick, if any, within delta of T (tick 0 is t0 itself, not
    rounded: it is never that tick).
    Returns, per query, the admissible segments of every tick (for check_tick_bounds)."""
    X, Y, PSI, K, V, A = (np.asarray(a, dtype=np.float64) for a in rows)
    Bn, N = X.shape
    hs = np.broadcast_to(np.asarray(h, dtype=np.float64), (Bn,))
    S = N if closed else N - 1
    Q = len(hz.seg)
    row = np.zeros(Q, dtype=np.int64) if row is None else np.asarray(row)
    fdt = F(float(dt))
    segs = []
    for q in range(Q):
        segs.append([])
        if int(hz.seg[q]) < 0:
            assert int(hz.count[q]) == 0, f"{label} query {q}: count {hz.count[q]} without a segment"
            continue
        b = int(row[q])
        t = np.asarray(stamps[b], dtype=np.float64)
        Tf = float(t[S])
        T, t0 = F(Tf), F(float(hz.t0[q]))
        count = int(hz.count[q])
        lab = f"{label} query {q}"
        if closed:
            want = m_cap if math.isfinite(Tf) and Tf > 0.0 else 0
            assert count == want, f"{lab}: count {count}, closed row with T {Tf!r}"
        else:
            below = [m for m in range(m_cap) if t0 + m * fdt < T]
            assert below == list(range(len(below)))
            edge = [m for m in range(1, m_cap) if abs(t0 + m * fdt - T) <= 4 * EPS * (t0 + m * fdt)]
            tally.add("count", bool(edge))
            if count != len(below):
                assert edge and abs(count - len(below)) == 1 and min(count, len(below)) in edge, \
                    f"{lab}: count {count}, {len(below)} ticks lie before T"
        for m in range(count):
            tau = t0 + m * fdt
            delta = 4 * EPS * tau if m else F(0)
            adm = _admissible(t, S, T, tau, delta, closed)
            assert adm, f"{lab} tick {m}: no segment holds tau* {float(tau)!r}"
            tally.ticks += 1
            tally.multi += len({i for _, i, _ in adm}) > 1
            slope = {}
            for _, i, _ in adm:
                j = (i + 1) % N
                dti = F(float(t[i + 1])) - F(float(t[i]))
                for n, a in zip(LERP_COLS, (X, Y, K, V)):
                    ai, aj = float(a[b, i]), float(a[b, j])
                    if math.isfinite(ai) and math.isfinite(aj):
                        slope[n] = max(slope.get(n, 0), abs(F(aj) - F(ai)) / dti)
                slope["s"] = max(slope.get("s", 0), abs(F(float(hs[b]))) / dti)
                slope["heading"] = max(slope.get("heading", 0),
                                       max(abs(d) for d in _arcs(float(PSI[b, i]), float(PSI[b, j]))[0]) / dti)
            why = []
            arc_seen = False
            for k, i, w in adm:
                j = (i + 1) % N
                u = (w - F(float(t[i]))) / (F(float(t[i + 1])) - F(float(t[i])))
                errs = [_lerp_check(tally, n, float(getattr(hz, n)[q, m]), float(a[b, i]), float(a[b, j]), u,
                                    slope.get(n, 0) * delta) for n, a in zip(LERP_COLS, (X, Y, K, V))]
                errs.append(_s_check(tally, float(hz.s[q, m]), k, S, i, u, hs[b], slope["s"] * delta))
                probe = Tally()
                errs.append(_heading_check(probe, float(hz.heading[q, m]), float(PSI[b, i]), float(PSI[b, j]), u,
                                           slope["heading"] * delta))
                arc_seen = arc_seen or probe.fired["arc"] > 0
                for key, val in probe.worst.items():
                    tally.worst[key] = max(tally.worst.get(key, 0.0), val)
                if not same_bits(hz.ax[q, m], A[b, i]):
                    errs.append(f"ax: {hz.ax[q, m]!r}, segment {i} has {A[b, i]!r}")
                errs = [e for e in errs if e]
                if not errs:
                    why = []
                    break
                why.append(f"lap {k} segment {i}: " + "; ".join(errs))
            tally.add("arc", arc_seen)
            assert not why, f"{lab} tick {m} at tau* {float(tau)!r}: no admissible segment explains it: " + " | ".join(why)
            segs[q].append(sorted({i for _, i, _ in adm}))
    return segs


# ---------------------------------------------------------------------------- the ticks' bounds
def _pair_bits(lo, hi, b, i, N):
    """The bit patterns the pair of segment i may have: the larger lo and the smaller hi of samples
    i and j = (i + 1) mod N (either pattern where the two compare equal)."""
    j = (i + 1) % N
    a, c = float(lo[b, i]), float(lo[b, j])
    d, e = float(hi[b, i]), float(hi[b, j])
    los = {int(bits([v])[0]) for v in (a, c) if v == max(a, c)}
    his = {int(bits([v])[0]) for v in (d, e) if v == min(d, e)}
    return los, his


def check_tick_bounds(hb, lo, hi, hz, row, segs, label=""):
    """lo0, hi0 bit-equal to the pair at seg; lo[q, m], hi[q, m] bit-equal to the pair of one and
    the same admissible segment of tick m (segs: check_horizon_ticks' return).  The pair is two
    selections, no arithmetic: nothing rounds."""
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)
    N = lo.shape[1]
    Q = len(hz.seg)
    row = np.zeros(Q, dtype=np.int64) if row is None else np.asarray(row)
    checked = 0
    for q in range(Q):
        i0, b = int(hz.seg[q]), int(row[q])
        if i0 < 0:
            continue
        los, his = _pair_bits(lo, hi, b, i0, N)
        assert int(bits(hb.lo0)[q]) in los and int(bits(hb.hi0)[q]) in his, \
            f"{label} query {q}: lo0, hi0 {hb.lo0[q]!r}, {hb.hi0[q]!r} are not the pair at segment {i0}"
        assert len(segs[q]) == int(hz.count[q])
        for m, adm in enumerate(segs[q]):
            gl, gh = int(bits(hb.lo)[q, m]), int(bits(hb.hi)[q, m])
            ok = False
            for i in adm:
                los, his = _pair_bits(lo, hi, b, i, N)
                ok = ok or (gl in los and gh in his)
            assert ok, (f"{label} query {q} tick {m}: lo, hi {hb.lo[q, m]!r}, {hb.hi[q, m]!r} are the pair of none of "
                        f"the admissible segments {adm}")
            checked += 1
    return checked


# ---------------------------------------------------------------------------- inputs and the drive
def shifted(rows, poses=None):
    """The rows with x + 4096 and y - 4096 (and the poses with them): far from the origin the
    subtractions of the foot cancel eleven or twelve leading bits."""
    out = (rows[0] + 4096.0, rows[1] - 4096.0) + tuple(rows[2:])
    if poses is None:
        return out
    return out, poses + np.array([4096.0, -4096.0])


def special_poses(rows, N, S, row):
    """Four poses on rows `row` [4] and their hints: exactly on sample 0, exactly on sample N - 1,
    far outside, about along the ray from the row's centroid through a sample (so that the nearest
    point is that vertex, shared by two segments), and a NaN pose."""
    X, Y = rows[0], rows[1]
    k = N // 2
    b = int(row[2])
    cx, cy = float(np.mean(X[b])), float(np.mean(Y[b]))
    rx, ry, a = X[b, k] - cx, Y[b, k] - cy, 0.5 / N                # (turned a little: at N = 2 the ray is the segment's line)
    far = [X[b, k] + 25.0 * (rx * math.cos(a) - ry * math.sin(a)), Y[b, k] + 25.0 * (rx * math.sin(a) + ry * math.cos(a))]
    P = np.array([[X[row[0], 0], Y[row[0], 0]], [X[row[1], N - 1], Y[row[1], N - 1]], far, [np.nan, 0.0]])
    hint = np.clip([0, N - 1, k, 0], 0, max(S - 1, 0)).astype(np.int32)
    return P, hint


def tick_variants(S, closed, hint, seg, t_max, m_few, m_many):
    """(label, hint, window, dt, m_cap) for the horizon: seg a typical segment's duration, t_max
    the longest row's; m_few ticks where the locate is the point, m_many where the ticks are."""
    Q = len(hint)
    v = [("no hint, several ticks per segment", None, 0, seg / 4.0, m_many),
         ("no hint, several segments per tick", None, 0, seg * 4.0, m_many),
         ("window 0", hint, 0, seg / 2.0, m_few),
         ("window 1", hint, 1, seg / 2.0, m_few),
         ("window >= S", hint, S + 3, seg / 2.0, m_few)]
    if closed:
        wrap = np.where(np.arange(Q) % 2 == 0, 0, S - 1).astype(np.int32)
        v += [("window across segment 0", wrap, min(3, S), seg / 2.0, m_few),
              ("more than two laps", None, 0, 2.5 * t_max / (m_many - 1), m_many)]
    else:
        v += [("window past the end of the row", np.full(Q, S - 1, dtype=np.int32), 2, seg / 2.0, m_few),
              ("the row ends first", None, 0, t_max / 4.0, 8),
              ("M_cap binds", None, 0, t_max / 1e4, 3)]
    return v


def drive(traj_fn, hzn_fn, bnd_fn, rows, h, closed, poses, row, hint, tally, m_few=2, m_many=6, feet=None, label=""):
    """One case through the three stages and every check of this module.  traj_fn and hzn_fn have
    the signatures of raceline.trajectory_host and raceline.horizon_host without `stamps`;
    bnd_fn(lo, hi, stamps, T, row, seg, t0, count, dt, m_cap, closed) that of horizon_bounds_host,
    or None where the tick kernel cannot be reached with given rows.  Returns what the tests
    assert on: the horizon results by label and the counts of what was checked."""
    X, V = np.asarray(rows[0]), np.asarray(rows[4])
    Bn, N = X.shape
    S = N if closed else N - 1
    hs = np.broadcast_to(np.asarray(h, dtype=np.float64), (Bn,))
    stamps = np.array([exact_stamps(V[b], hs[b]) for b in range(Bn)])
    done = dict(traj_ticks=0, bound_ticks=0, hzn={})
    if S < 1:
        tr = traj_fn(*rows, h, closed, 0.1, 4)
        done["traj_ticks"] += check_trajectory(tr, rows, h, closed, 0.1, 4, tally, label=label)
        hz = hzn_fn(*rows, h, closed, poses, row=row, dt=0.1, m_cap=4)
        check_locate(hz, rows, stamps, h, closed, poses, row, None, 0, tally, label=label)
        assert np.all(hz.seg == -1) and np.all(hz.count == 0)
        return done
    durs = np.diff(stamps[:, :S + 1], axis=1)
    seg = float(np.mean(durs[durs > 0]))
    t_min, t_max = float(np.min(stamps[:, S])), float(np.max(stamps[:, S]))
    on_stamp = float(stamps[0, min(2, S)])                          # a tick exactly on a stamp of row 0
    for what, dt, m_cap in (("several ticks per segment", seg / 3.0, 4 * m_few), ("several segments per tick", seg * 4.0, 4 * m_few),
                            ("the row ends first", t_min / 3.5, 8), ("M_cap binds", t_min / 1e4, 3),
                            ("a tick on a stamp", on_stamp, 3)):
        tr = traj_fn(*rows, h, closed, dt, m_cap)
        n = check_trajectory(tr, rows, h, closed, dt, m_cap, tally, label=f"{label} trajectory, {what}")
        done["traj_ticks"] += n
        if what == "the row ends first":
            assert np.min(tr.count) == 4 and np.min(tr.count) < m_cap
        if what == "M_cap binds":
            assert np.all(tr.count == m_cap)
    feet = {} if feet is None else feet
    rng = np.random.default_rng(N)
    lo, hi = -rng.uniform(0.1, 2.0, size=X.shape), rng.uniform(0.1, 2.0, size=X.shape)
    variants = tick_variants(S, closed, hint, seg, t_max, m_few, m_many)
    k = 0
    while k < len(variants):
        what, hn, W, dt, m_cap = variants[k]
        lab = f"{label} horizon, {what}"
        hz = hzn_fn(*rows, h, closed, poses, row=row, seg_hint=hn, window=W, dt=dt, m_cap=m_cap)
        done["hzn"][what] = hz
        check_locate(hz, rows, stamps, h, closed, poses, row, hn, W, tally, feet, lab)
        segs = check_horizon_ticks(hz, rows, stamps, h, closed, row, dt, m_cap, tally, lab)
        if bnd_fn is not None:
            hb = bnd_fn(lo, hi, stamps, stamps[:, S], row, hz.seg, hz.t0, hz.count, dt, m_cap, closed)
            done["bound_ticks"] += check_tick_bounds(hb, lo, hi, hz, row, segs, lab)
        if k == 0:
            # the nearest segment at the very edge of a window of 2: a window one short loses it
            g = np.where(hz.seg < 0, 0, (hz.seg - 2) % S if closed else np.maximum(hz.seg - 2, 0)).astype(np.int32)
            variants.append(("the nearest segment at the window's edge", g, 2, seg / 2.0, m_few))
        k += 1
    return done
