"""An exact-arithmetic reference of the recover family: the recover stage (rl_recover.hip and the
device functions of rl_recover.h) and the fan stage (rl_recover_fan.hip).  A plain helper module
like resample_exact, whose locate check and tally it reuses: no fixtures, no pytest settings.

The operations are stated here from the words of include/rl_abi.h (the recover and fan blocks) and
DESIGN 3q / 3r in rational arithmetic (fractions.Fraction; every double converts exactly) with
linear scans only.  From raceline.py nothing is imported but the result classes' fields, read off
the answer that is checked.  What a stage returns (raceline.recover_host or raceline.recover,
recover_fan_host or recover_fan, or a plan's fetch) is checked against these statements within
bounds that follow from counting the roundings of the contract's formulas; each derivation stands
in the docstring of the helper that applies it.  EPS = 2**-53 is the unit roundoff: one operation
returns its exact result times (1 + d), |d| <= EPS.  Terms of order EPS**2 are covered by the room
between the counted roundings and the constants used, and where a bound divides by a perturbed
quantity, by the factor 1 / (1 - rho) written there.

The speed pass (ceiling, envelope, march: node_b, node_v, node_t, feasible, overspeed, v_excess,
bind_node, t_loss) is the retime stage's and stays anchored there (DESIGN 3p, and 3q's anchor
e == 0); here the hand-over to it is checked (node_c from the returned node_k), and everything the
stage derives from the march's node_t and node_v afterwards (t_end, count, the ticks).

Skipped checks, each counted per kind in the Tally (resample_exact's kinds and four more):
    slope       den, |num| - den or num within the counted bound of 0: the branch of g0 is not
                defined by the data; the query's offsets and clamp count are then not compared
    merge       some a_k within 4 EPS a_k of D: merge_node is not defined by the data
    clamp       a node whose raw* is within the counted bound of lo or hi (counted, never skipped:
                it widens the bracket of `clamped`)
    degenerate  a Menger node or a chord whose relative perturbation rho reaches 1/2
    arc         two node headings within 2**-50 (and their own bounds) of half a turn apart
"""
import math
from fractions import Fraction as F

import numpy as np

import resample_exact as RX
from resample_exact import EPS, PI, TWO_PI, bits, same_bits

ULP_PI = F(1, 2 ** 51)                   # one ulp of a double in [2, 4): math.atan2's error at most
HALF_ULP_PI = F(1, 2 ** 52)              # atan2_cr's
LOC_FIELDS = ("seg", "u", "e", "dist2", "t0", "s0")


class Tally(RX.Tally):
    KINDS = RX.Tally.KINDS + ("slope", "merge", "clamp", "degenerate")

    def __init__(self):
        super().__init__()
        self.items = dict.fromkeys(self.KINDS, 0)
        self.fired = dict.fromkeys(self.KINDS, 0)
        self.nodes = 0
        self.queries = 0
        self.slopes = {-1: 0, 0: 0, 1: 0}   # queries by the sign of the exact g0

    def add_n(self, kind, items, fired):
        self.items[kind] += items
        self.fired[kind] += fired


def fsqrt(q, prec=160):
    """sqrt of a Fraction q >= 0 to a relative 2**-prec/2 or better, as a Fraction (integer square root)."""
    if q == 0:
        return F(0)
    p, d = q.numerator, q.denominator
    s = max(0, prec - (p * d).bit_length() // 2)
    return F(math.isqrt(p * d << (2 * s)), d << s)


def _norm(x, y):
    return fsqrt(x * x + y * y)


def q_poly(z):
    """q(z) = 1 - 10 z^3 + 15 z^4 - 6 z^5: value 1 at 0, 0 at 1, no slope or second derivative at either."""
    return 1 - 10 * z ** 3 + 15 * z ** 4 - 6 * z ** 5


def p_poly(z):
    """p(z) = z - 6 z^3 + 8 z^4 - 3 z^5: slope 1 at 0, every other value, slope and second derivative 0."""
    return z - 6 * z ** 3 + 8 * z ** 4 - 3 * z ** 5


# counted below, in exact_offsets' docstring
Q_ERR = 77 * EPS + F(15, 8) * 4 * EPS
P_ERR = 44 * EPS + 4 * EPS


# ---------------------------------------------------------------------------- slope
def exact_slope(dx, dy, hx, hy):
    """(g0*, bg, defined) for the segment direction (dx, dy) = P_j - P_i, exact, and the car's (hx, hy).

    den* = dx hx + dy hy, num* = dx hy - dy hx.  The kernel rounds dx and dy once each, each
    product once and the sum once: |den^ - den*| <= 3 EPS (|dx hx| + |dy hy|) and the same for
    num with (|dx hy| + |dy hx|); bden, bnum take 4 EPS of those.  The branch den > 0 is the exact
    one unless |den*| <= bden; inside it the clamp to +-1 is the exact one unless
    ||num*| - den*| <= bnum + bden, outside it the sign of num unless |num*| <= bnum: each of
    those leaves defined = False.  Clamped or by sign, g0 is +-1 or 0 exactly: bg = 0.  Otherwise
    g0^ = fl(num^ / den^), |num^ / den^ - num* / den*| <= (bnum + |g0*| bden) / (den* - bden), and
    the quotient's own rounding EPS |g0^| <= EPS (with |g0| <= 1)."""
    den, num = dx * hx + dy * hy, dx * hy - dy * hx
    bden, bnum = 4 * EPS * (abs(dx * hx) + abs(dy * hy)), 4 * EPS * (abs(dx * hy) + abs(dy * hx))
    if abs(den) <= bden:
        return F(0), F(0), False
    if den > 0:
        if abs(abs(num) - den) <= bnum + bden:
            return F(0), F(0), False
        if abs(num) > den:
            return F(1 if num > 0 else -1), F(0), True
        g = num / den
        return g, (bnum + abs(g) * bden) / (den - bden) + EPS, True
    if abs(num) <= bnum and num != 0:
        return F(0), F(0), False
    return F(0 if num == 0 else (1 if num > 0 else -1)), F(0), True


# ---------------------------------------------------------------------------- offsets
def exact_offsets(e, g0, bg, D, u, h, K):
    """[(a_k*, raw_k*, braw_k)] for k = 1 .. K, from the returned e and u.

    a_k* = (1 - u) h + (k - 1) h.  The kernel has d0^ = fl(fl(1 - u) h) (two roundings),
    fl((k - 1) h) (one; k - 1 is exact) and their sum (one); all terms are positive, so
    a^ = a* (1 + 3 EPS), and z^ = smin(1, fl(a^ / D)) is within 4 EPS z* <= 4 EPS of
    z* = min(1, a* / D): the clamp to 1 does not widen a distance.
    q in Horner form at z^ in [0, 1]: fl(6 z) <= 6 carries 6 EPS; 15 - . in [9, 15]: 6 + 15 = 21
    EPS; z * . <= 15: 21 + 15 = 36 EPS; -10 + . in [-10, -1]: 36 + 10 = 46 EPS; z3 = fl(fl(z z) z)
    carries 2 EPS z3; z3 * . <= 10 z3: the factor's 46 EPS times z3 <= 1, z3's 2 EPS times 10 and
    the product's own rounding of 10 EPS give 46 + 20 + 10 = 76 EPS; 1 + . in [0, 1]: 77 EPS.
    |q'| = 30 z^2 (1 - z)^2 <= 15 / 8 moves that by 15/8 * 4 EPS for z^ against z*: Q_ERR.
    p alike: fl(3 z): 3 EPS; 8 - . in [5, 8]: 11; z * . <= 8: 19; -6 + . in [-6, -1]: 25; z3 * .
    <= 6 z3: 25 + 12 + 6 = 43; z + . in [0, 1]: 44 EPS; |p'| <= 1: 4 EPS more: P_ERR.
    raw^ = fl(fl(e qz^) + fl(gD^ pz^)) with gD^ = fl(g0^ D): the first product is within
    |e| (Q_ERR + EPS) of e q*; gD^ within D (bg + EPS |g0*|) of g0* D, so the second is within
    |g0*| D (P_ERR + 2 EPS |p*|) + D bg (|p*| + P_ERR) of g0* D p*; the sum rounds once more,
    EPS (|e q*| + |g0* D p*|) <= EPS |e| + EPS |g0*| D |p*|:
        braw = |e| (Q_ERR + 2 EPS) + |g0*| D (P_ERR + 3 EPS |p*|) + D bg (|p*| + P_ERR).
    At z* = 1 with a* clear of D, z^ = 1 too and both polynomials are exactly 0: merge_node's
    own check covers that; braw is not used there."""
    out = []
    for k in range(1, K + 1):
        a = (1 - u) * h + (k - 1) * h
        z = min(F(1), a / D)
        qz, pz = q_poly(z), p_poly(z)
        raw = e * qz + g0 * D * pz
        braw = abs(e) * (Q_ERR + 2 * EPS) + abs(g0) * D * (P_ERR + 3 * EPS * abs(pz)) + D * bg * (abs(pz) + P_ERR)
        out.append((a, raw, braw))
    return out


def exact_clamp(raw, lo, hi):
    """smin(hi, smax(lo, raw)) in words: the larger of lo and raw, then the smaller of that and hi
    (so hi where lo > hi).  lo, hi finite."""
    return min(hi, max(lo, raw))


# ---------------------------------------------------------------------------- one query
class _Query:
    pass


def _pair(lo, hi, b, i, N):
    return RX._pair_bits(lo, hi, b, i, N)


def _lerp(tally, name, got, A, Bv, u, slack):
    """got against A + u (B - A), A and B exact: resample_exact._lerp_check's count, 8 EPS (|A| + |B|)
    for the three roundings of u^, the difference, the product and the sum, and the caller's slack
    for what the kernel's own A^ and B^ differ from A and B by."""
    if not math.isfinite(got):
        return f"{name}: {got!r}"
    exact = A + u * (Bv - A)
    room = 8 * EPS * (abs(A) + abs(Bv)) + slack
    err = abs(F(got) - exact)
    if err <= room:
        tally.ratio(name, err, room)
        return None
    return f"{name}: {got!r}, exact {float(exact)!r}, off by {float(err):.3e} > {float(room):.3e}"


def check_query(rc, q, rows, h, closed, lo, hi, nx, ny, pose, D, H, b, cfg, dt, m_cap, k_cap, tally, label=""):
    """Everything after the locate for one answered query q of a Recover `rc` on row b.

    Points.  P_k* = (x_n + o_k nx_n, y_n + o_k ny_n) from the returned o_k, n = (seg + k) mod N;
    P_0* is the pose.  The kernel's P_k^ = fl(x + fl(o nx)): EPS |o nx| for the product and
    EPS (|x| + |o nx|) for the sum, with |nx| <= 1 + EPS: at most 2 EPS (|x| + |o|) per coordinate
    (bP).  P_0^ = X0 + r with X0 = fl(x_i + fl(u fl(dx))) and r = fl(fl(wx) - fl(u fl(dx))): seven
    roundings of values up to |x_i| + |p| + |dx|: bP_0 = 8 EPS (|x_i| + |p_x| + |dx|); tick 0 is
    held to 2 ulp of the pose besides, DESIGN 3q's own words (per coordinate: an ulp of the largest of
    |p_x|, |x_i| and |x_j|, between which the foot X0 lies, for x; the same with y for y).
    Chords.  q = P_{k+1} - P_k: the kernel's differs by the two points' errors and one rounding,
    dq <= bP_k + bP_{k+1} + EPS |q| per coordinate; d'^ = sqrt(fl(qx qx + qy qy)) carries 2 EPS
    more (product and sum, then the root halves 2 EPS and rounds once).  With |dq| the 1-norm of
    the coordinates' errors: |d'^ - d'*| <= |dq| + 2 EPS d'*, relatively rho_d = |dq| / d'* + 2 EPS.
    A segment on the line (o_k == o_{k+1} == 0) has d' = d_k: h itself, or d_0 = fl(fl(1 - u) h),
    2 EPS.
    Menger.  kappa* = 2 cross(a*, b*) / (d'*_{k-1} d'*_k |c*|) with a, b, c the exact chords and
    d'* as the contract has it (a chord, or d_k on the line).  cross^ = fl(fl(ax by) - fl(ay bx)):
    |cross(a + da, b + db) - cross(a, b)| <= |da| |b| + |a| |db| + |da| |db| and the three
    roundings give 3 EPS (|ax by| + |ay bx|) <= 3 EPS |a| |b| (Cauchy-Schwarz): bcross.  This is
    where the cancellation sits: for nearly collinear nodes cross is small and bcross is not, and
    the bound is absolute, 2 bcross / den*, so no skip is needed.  den^ is the product of three
    lengths with relative errors rho_a, rho_b, rho_c (above) and two products' roundings, the
    quotient one more: rho = rho_a + rho_b + rho_c + 4 EPS, and
        |kappa^ - kappa*| <= (2 bcross / den* + |kappa*| rho) / (1 - rho).
    Headings.  A node off the line has psi = atan2 of its chord c (across it, or its one segment
    at an end): the exact chord rounded to double moves the angle by at most EPS per coordinate
    (2 EPS), math.atan2 by one ulp (2**-51 below pi); the kernel's chord differs by |dc| / |c|
    radians and atan2_cr rounds by half an ulp: bpsi = |dc| / |c| + 2 EPS + 2**-51 + 2**-52.  A node
    on the line has the row's heading (node 0: interpolated along the shorter arc with u,
    8 EPS (|psi_i| + |psi_j| + 2 pi) as resample_exact counts it)."""
    X, Y, PSI, KAP, V, _ = (np.asarray(a, dtype=np.float64)[b] for a in rows)
    N = X.shape[0]
    lab = f"{label} query {q}"
    i0, K = int(rc.seg[q]), int(rc.end_node[q])
    j0 = (i0 + 1) % N
    room = N if closed else N - 1 - i0
    assert K == min(k_cap, room), f"{lab}: end_node {K}, K_cap {k_cap}, room {room}"
    uf, ef = float(rc.u[q]), float(rc.e[q])
    u, e, hq, Dq = F(uf), F(ef), F(float(h)), F(float(D))
    o = [float(v) for v in rc.node_o[q, :K + 1]]
    kp = [float(v) for v in rc.node_k[q, :K + 1]]
    tt = [float(v) for v in rc.node_t[q, :K + 1]]
    w = [float(v) for v in rc.node_v[q, :K + 1]]
    n = [(i0 + k) % N for k in range(K + 1)]
    LO, HI = np.asarray(lo, dtype=np.float64)[b], np.asarray(hi, dtype=np.float64)[b]
    NX, NY = np.asarray(nx, dtype=np.float64)[b], np.asarray(ny, dtype=np.float64)[b]
    tally.queries += 1
    tally.nodes += K + 1

    # ---- slope and offsets
    assert same_bits(o[0], ef), f"{lab}: node_o[0] {o[0]!r} != e {ef!r}"
    dxs, dys = F(float(X[j0])) - F(float(X[i0])), F(float(Y[j0])) - F(float(Y[i0]))
    if H is None:
        g0, bg, defined = F(0), F(0), True
    else:
        g0, bg, defined = exact_slope(dxs, dys, F(float(H[0])), F(float(H[1])))
        tally.add("slope", not defined)
        if defined:
            tally.slopes[(g0 > 0) - (g0 < 0)] += 1
    prof = exact_offsets(e, g0, bg, Dq, u, hq, K)
    near = [k for k, (a, _, _) in enumerate(prof, 1) if abs(a - Dq) <= 4 * EPS * a]
    tally.add("merge", bool(near))
    mg = int(rc.merge_node[q])
    if not near:
        first = next((k for k, (a, _, _) in enumerate(prof, 1) if a >= Dq), -1)
        assert mg == first, f"{lab}: merge_node {mg}, the first a_k* >= D is node {first}"
    certain = ambiguous = 0
    for k, (a, raw, braw) in enumerate(prof, 1):
        lk, hk = float(LO[n[k]]), float(HI[n[k]])
        if math.isnan(lk) or math.isnan(hk):
            continue
        if lk <= hk:
            assert lk <= o[k] <= hk, f"{lab}: node_o[{k}] {o[k]!r} outside {lk!r} .. {hk!r} of sample {n[k]}"
        if mg >= 0 and k >= mg and lk <= 0.0 <= hk:
            assert o[k] == 0.0, f"{lab}: node_o[{k}] {o[k]!r} at or past merge_node {mg}"
        if H is None and ef == 0.0 and lk <= 0.0 <= hk:
            assert o[k] == 0.0, f"{lab}: node_o[{k}] {o[k]!r} for a car on the line heading along it"
        if not defined:
            continue
        want = exact_clamp(raw, F(lk), F(hk))
        err = abs(F(o[k]) - want)
        assert err <= braw, (f"{lab}: node_o[{k}] {o[k]!r}, the clamped profile is {float(want)!r} (raw {float(raw)!r}, "
                             f"lo {lk!r}, hi {hk!r}): off by {float(err):.3e} > {float(braw):.3e}")
        tally.ratio("node_o", err, braw)
        edge = abs(raw - F(lk)) <= braw or abs(raw - F(hk)) <= braw
        if edge:
            ambiguous += 1
        elif want != raw:
            certain += 1
    tally.add_n("clamp", K, ambiguous)
    if defined and not np.isnan(LO[n[1:]]).any() and not np.isnan(HI[n[1:]]).any():
        cl = int(rc.clamped[q])
        assert certain <= cl <= certain + ambiguous, f"{lab}: clamped {cl}, certainly {certain}, ambiguous {ambiguous}"

    # ---- the car's room
    los, his = _pair(np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64), b, i0, N)
    assert int(bits(rc.lo0)[q]) in los and int(bits(rc.hi0)[q]) in his, \
        f"{lab}: lo0, hi0 {rc.lo0[q]!r}, {rc.hi0[q]!r} are not the pair of segment {i0}"
    assert int(rc.offtrack[q]) == (0 if float(rc.lo0[q]) <= ef <= float(rc.hi0[q]) else 1), f"{lab}: offtrack {rc.offtrack[q]}"

    # ---- points
    px, py = F(float(pose[0])), F(float(pose[1]))
    Px, Py, bPx, bPy = [px], [py], [8 * EPS * (abs(F(float(X[i0]))) + abs(px) + abs(dxs))], \
        [8 * EPS * (abs(F(float(Y[i0]))) + abs(py) + abs(dys))]
    for k in range(1, K + 1):
        xo, yo, ok = F(float(X[n[k]])), F(float(Y[n[k]])), F(o[k])
        Px.append(xo + ok * F(float(NX[n[k]])))
        Py.append(yo + ok * F(float(NY[n[k]])))
        bPx.append(2 * EPS * (abs(xo) + abs(ok)))
        bPy.append(2 * EPS * (abs(yo) + abs(ok)))
    def chord(a, c):
        """(cx, cy, |c|, |dc| in the 1-norm) of P_c - P_a."""
        cx, cy = Px[c] - Px[a], Py[c] - Py[a]
        dc = bPx[a] + bPx[c] + EPS * abs(cx) + bPy[a] + bPy[c] + EPS * abs(cy)
        return cx, cy, _norm(cx, cy), dc

    # "Segment k is on the line if o_k == 0.0 && o_{k+1} == 0.0: d'_k = d_k.  Otherwise d'_k = |P_{k+1} - P_k|."
    d0 = (1 - u) * hq
    seg = []                              # (d'*, rho_d) per segment
    for k in range(K):
        if o[k] == 0.0 and o[k + 1] == 0.0:
            seg.append((d0 if k == 0 else hq, 2 * EPS if k == 0 else F(0)))
        else:
            _, _, ln, dc = chord(k, k + 1)
            seg.append((ln, dc / ln + 2 * EPS if ln > 0 else None))

    # "Node k is on the line if o_m == 0.0 for every m of {k-1, k, k+1} within [0, K]"
    node_on_line = [all(o[m] == 0.0 for m in (k - 1, k, k + 1) if 0 <= m <= K) for k in range(K + 1)]

    # ---- curvatures
    for k in range(K + 1):
        if node_on_line[k]:
            # "kappa'_k = kappa_k": the row's at sample n_k; node 0's is interpolated on the located segment
            if k:
                assert same_bits(kp[k], float(KAP[n[k]])), f"{lab}: node_k[{k}] {kp[k]!r} on the line, the row has {KAP[n[k]]!r}"
            else:
                bad = _lerp(tally, "node_k[0]", kp[0], F(float(KAP[i0])), F(float(KAP[j0])), u, 0)
                assert not bad, f"{lab}: {bad}"
        elif 1 <= k <= K - 1:
            # "a = P_k - P_{k-1}, b = P_{k+1} - P_k, c = P_{k+1} - P_{k-1}: den = (d'_{k-1} d'_k) |c|,
            #  kappa'_k = den > 0 ? 2 (ax by - ay bx) / den : 0.0"
            a1, a2, la, da = chord(k - 1, k)
            b1, b2, lb, db = chord(k, k + 1)
            _, _, lc, dc = chord(k - 1, k + 1)
            den = seg[k - 1][0] * seg[k][0] * lc
            if den == 0:
                assert kp[k] == 0.0, f"{lab}: node_k[{k}] {kp[k]!r} with a vanishing denominator"
                continue
            rho = (seg[k - 1][1] or 0) + (seg[k][1] or 0) + dc / lc + 2 * EPS + 4 * EPS
            bad = seg[k - 1][1] is None or seg[k][1] is None or rho >= F(1, 2)
            tally.add("degenerate", bad)
            if bad:
                continue
            kap = 2 * (a1 * b2 - a2 * b1) / den
            bcross = da * lb + la * db + da * db + 3 * EPS * la * lb
            bound = (2 * bcross / den + abs(kap) * rho) / (1 - rho)
            err = abs(F(kp[k]) - kap) if math.isfinite(kp[k]) else None
            assert err is not None and err <= bound, (f"{lab}: node_k[{k}] {kp[k]!r}, Menger through the exact points gives "
                                                      f"{float(kap)!r}: off by {float(err or 0):.3e} > {float(bound):.3e}")
            tally.ratio("node_k", err, bound)
        elif K >= 2:
            # "End nodes off the line: kappa'_0 = kappa'_1 and kappa'_K = kappa'_{K-1} when K >= 2"
            nb = 1 if k == 0 else K - 1
            assert same_bits(kp[k], kp[nb]), f"{lab}: end node_k[{k}] {kp[k]!r} is not its neighbour's {kp[nb]!r}"
        elif k:
            # "otherwise the row's"
            assert same_bits(kp[k], float(KAP[n[k]])), f"{lab}: node_k[{k}] {kp[k]!r} at K = 1, the row has {KAP[n[k]]!r}"
        else:
            bad = _lerp(tally, "node_k[0]", kp[0], F(float(KAP[i0])), F(float(KAP[j0])), u, 0)
            assert not bad, f"{lab}: {bad}"

    # ---- the ceiling's hand-over
    vcap, alat, keps = float(cfg.v_cap_mps), float(cfg.a_lat_max), float(cfg.kappa_eps)
    for k in range(K + 1):
        r = float(V[n[k]]) if k else float(V[i0]) + uf * (float(V[j0]) - float(V[i0]))
        ak = abs(kp[k])
        c = math.sqrt(alat / (keps if ak < keps else ak))
        c = c if c < vcap else vcap
        c = r if r < c else c
        assert same_bits(rc.node_c[q, k], c), f"{lab}: node_c[{k}] {rc.node_c[q, k]!r}, the ceiling of node_k and r is {c!r}"

    # ---- node headings
    # on the line "psi_k is the rejoin stage's node heading"; off it psi_k = atan2(c) for 1 <= k <= K-1,
    # "psi_0 = atan2_cr of P_1 - P_0, psi_K = atan2_cr of P_K - P_{K-1}"
    psi, bpsi = [], []
    for k in range(K + 1):
        if node_on_line[k] and k:
            psi.append(F(float(PSI[n[k]])))
            bpsi.append(F(0))
        elif node_on_line[k]:
            pi_, pj = F(float(PSI[i0])), F(float(PSI[j0]))
            d = pj - pi_
            d = d - TWO_PI if d > PI else d + TWO_PI if d < -PI else d
            psi.append(pi_ + u * d)
            bpsi.append(8 * EPS * (abs(pi_) + abs(pj) + TWO_PI))
        else:
            cx, cy, lc, dc = chord(0, 1) if k == 0 else chord(K - 1, K) if k == K else chord(k - 1, k + 1)
            psi.append(F(math.atan2(float(cy), float(cx))))
            bpsi.append((dc / lc if lc > 0 else F(4)) + 2 * EPS + ULP_PI + HALF_ULP_PI)

    # ---- ticks
    assert same_bits(rc.t_end[q], tt[K]), f"{lab}: t_end {rc.t_end[q]!r} != node_t[K] {tt[K]!r}"
    count = RX.tick_count(tt[K], dt, m_cap)
    assert int(rc.count[q]) == count, f"{lab}: count {rc.count[q]}, the scan gives {count}"
    rising = all(tt[k] < tt[k + 1] for k in range(K))
    a = 0
    for m in range(count):
        tau = float(m) * dt
        if rising:
            while not (tt[a] <= tau < tt[a + 1]):          # the linear scan: tau does not decrease with m
                a += 1
            hits = [a]                                     # (the only one: node_t rises strictly)
        else:
            hits = [k for k in range(K) if tt[k] <= tau < tt[k + 1]]
        assert hits, f"{lab} tick {m}: no interval of node_t holds tau {tau!r}"
        why = []
        for k in hits:
            um = (F(tau) - F(tt[k])) / (F(tt[k + 1]) - F(tt[k]))
            errs = [_lerp(tally, "x", float(rc.x[q, m]), Px[k], Px[k + 1], um, max(bPx[k], bPx[k + 1])),
                    _lerp(tally, "y", float(rc.y[q, m]), Py[k], Py[k + 1], um, max(bPy[k], bPy[k + 1])),
                    _lerp(tally, "kappa", float(rc.kappa[q, m]), F(kp[k]), F(kp[k + 1]), um, 0),
                    _lerp(tally, "v", float(rc.v[q, m]), F(w[k]), F(w[k + 1]), um, 0),
                    _lerp(tally, "offset", float(rc.offset[q, m]), F(o[k]), F(o[k + 1]), um, 0)]
            # s: sa = fl(fl(i0 + u) h) (node 0) or fl((i0 + a) h), sb = fl((i0 + a + 1) h): 2 EPS sa and EPS sb
            sa, sb = ((i0 + u) if k == 0 else F(i0 + k)) * hq, F(i0 + k + 1) * hq
            errs.append(_lerp(tally, "s", float(rc.s[q, m]), sa, sb, um, 2 * EPS * (sa + sb)))
            # ax = fl(fl(fl(wb wb) - fl(wa wa)) / fl(2 d'^)): 2 EPS (wa^2 + wb^2) in the numerator, rho_d in d', EPS the quotient
            dk, rho = seg[k]
            got = float(rc.ax[q, m])
            if dk == 0:
                if got != 0.0:
                    errs.append(f"ax: {got!r} on a segment of no length")
            elif rho is None or rho >= F(1, 2):
                tally.add("degenerate", True)
            else:
                wa2, wb2 = F(w[k]) ** 2, F(w[k + 1]) ** 2
                exact = (wb2 - wa2) / (2 * dk)
                bound = (2 * EPS * (wa2 + wb2) / (2 * dk) + abs(exact) * (rho + EPS)) / (1 - rho)
                err = abs(F(got) - exact) if math.isfinite(got) else None
                if err is None or err > bound:
                    errs.append(f"ax: {got!r}, exact {float(exact)!r}, allowed {float(bound):.3e}")
                else:
                    tally.ratio("ax", err, bound)
            # heading: resample_exact._heading_check's count, with the two nodes' own bounds as slack
            slack = bpsi[k] + bpsi[k + 1]
            d = psi[k + 1] - psi[k]
            short = d - TWO_PI if d > PI else d + TWO_PI if d < -PI else d
            near_pi = abs(abs(d) - PI) <= RX.ARC_NEAR + slack
            tally.add("arc", near_pi)
            arcs = [short, short - TWO_PI if short > 0 else short + TWO_PI] if near_pi else [short]
            hroom = 8 * EPS * (abs(psi[k]) + abs(psi[k + 1]) + TWO_PI) + slack
            got = float(rc.heading[q, m])
            best = None
            for dd in arcs:
                diff = F(got) - (psi[k] + um * dd) if math.isfinite(got) else None
                r_ = None if diff is None else abs(diff - round(diff / TWO_PI) * TWO_PI)
                if r_ is not None and (best is None or r_ < best):
                    best = r_
            if best is None or best > hroom:
                errs.append(f"heading: {got!r} is {float(best or 0):.3e} from the shorter arc modulo 2 pi, allowed {float(hroom):.3e}")
            else:
                tally.ratio("heading", best, hroom)
            errs = [x for x in errs if x]
            if not errs:
                why = []
                break
            why.append(f"interval {k}: " + "; ".join(errs))
        assert not why, f"{lab} tick {m} at tau {tau!r}: " + " | ".join(why)
        tally.ticks += 1
    if count:
        # P_0 = X0 + r: X0 = fl(x_i + u dx) lies between x_i and x_j and rounds at its own size, the sum at the pose's
        for name, p, ends in (("x", float(pose[0]), (float(X[i0]), float(X[j0]))), ("y", float(pose[1]), (float(Y[i0]), float(Y[j0])))):
            got = float(getattr(rc, name)[q, 0])
            big = max(abs(p), abs(ends[0]), abs(ends[1]))
            assert abs(F(got) - F(p)) <= 2 * F(math.ulp(big)), f"{lab}: tick 0 {name} {got!r} is not within 2 ulp of the pose's {p!r}"


# ---------------------------------------------------------------------------- a whole answer
def check_recover(rc, rows, h, closed, lo, hi, nx, ny, poses, cfg, D, dir_xy, row, dt, m_cap, k_cap, tally,
                  queries=None, hint=None, window=0, label=""):
    """A Recover answer for Q poses: resample_exact.check_locate on all of them (the HZN_LOC
    fields against stamps stated exactly from the rows' v), then check_query on `queries` (None:
    every one).  An unanswered query (a NaN pose, an open row's last sample) has end_node = -1 and
    count = 0.  Returns the number of queries checked in full."""
    X, V = np.asarray(rows[0], dtype=np.float64), np.asarray(rows[4], dtype=np.float64)
    Bn, N = X.shape
    hs = np.broadcast_to(np.asarray(h, dtype=np.float64), (Bn,))
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 2)
    Q = P.shape[0]
    row = np.zeros(Q, dtype=np.int64) if row is None else np.asarray(row)
    Dq = np.broadcast_to(np.asarray(D, dtype=np.float64), (Q,))
    stamps = np.array([RX.exact_stamps(V[b], hs[b]) for b in range(Bn)])

    class Loc:                                                      # check_locate's count of an unanswered query is 0 here too
        pass
    loc = Loc()
    for f in LOC_FIELDS + ("count",):
        setattr(loc, f, getattr(rc, f))
    RX.check_locate(loc, rows, stamps, hs, closed, P, row, hint, window, tally, label=label)
    done = 0
    for q in (range(Q) if queries is None else queries):
        i0 = int(rc.seg[q])
        room = 0 if i0 < 0 else (N if closed else N - 1 - i0)
        if min(k_cap, room) < 1:
            assert int(rc.end_node[q]) == -1 and int(rc.count[q]) == 0, f"{label} query {q}: end_node {rc.end_node[q]}, count {rc.count[q]} without a node ahead"
            continue
        Hq = None if dir_xy is None else np.asarray(dir_xy, dtype=np.float64).reshape(-1, 2)[q if np.ndim(dir_xy) == 2 else 0]
        check_query(rc, q, rows, hs[int(row[q])], closed, lo, hi, nx, ny, P[q], Dq[q], Hq, int(row[q]), cfg, float(dt), int(m_cap),
                    int(k_cap), tally, label)
        done += 1
    return done


# ---------------------------------------------------------------------------- the fan
TABLE = (("cand_feasible", "feasible"), ("cand_clamped", "clamped"), ("cand_merge_node", "merge_node"),
         ("cand_overspeed", "overspeed"), ("cand_bind_node", "bind_node"), ("cand_t_end", "t_end"), ("cand_t_loss", "t_loss"),
         ("cand_v_excess", "v_excess"))


def fan_class(feasible, clamped, merge_node):
    """DESIGN 3r's words: 0 = feasible, not clamped and merged; 1 = feasible and merged; 2 = feasible; 3 = otherwise."""
    if feasible and clamped == 0 and merge_node >= 0:
        return 0
    if feasible and merge_node >= 0:
        return 1
    return 2 if feasible else 3


def check_fan(fan, one_fn, rows, h, closed, lo, hi, nx, ny, poses, cfg, lengths, dir_xy, row, dt, m_cap, k_cap, tally,
              queries=None, label=""):
    """A RecoverFan answer.  one_fn(D [Q]) answers the recover stage for one length per query
    (raceline.recover_host or raceline.recover with everything else bound): every candidate's
    answer is checked by check_recover and table row c must hold its per-query values bit for bit;
    cand_class from fan_class; best the first in (class, isnan(t_end), t_end, c) by a linear scan
    over the returned cand_t_end; the winner's fields by check_recover with the winning length, and
    bit-equal to the candidate's where both are returned."""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 2)
    Q = P.shape[0]
    L = np.asarray(lengths, dtype=np.float64)
    L = np.broadcast_to(L, (Q, L.shape[-1]))
    Cn = L.shape[1]
    qs = list(range(Q)) if queries is None else list(queries)
    ok = fan.end_node >= 0
    singles = []
    for c in range(Cn):
        one = one_fn(np.ascontiguousarray(L[:, c]))
        check_recover(one, rows, h, closed, lo, hi, nx, ny, P, cfg, L[:, c], dir_xy, row, dt, m_cap, k_cap, tally, qs,
                      label=f"{label} candidate {c}")
        for f, src in TABLE:
            g, wv = getattr(fan, f)[ok, c], getattr(one, src)[ok]
            assert np.array_equal(bits(g.astype(np.float64)), bits(wv.astype(np.float64))), f"{label}: {f}[{c}] is not the recover stage's {src}"
        singles.append(one)
    for q in range(Q):
        if not ok[q]:
            assert int(fan.best[q]) == -1 and int(fan.count[q]) == 0, f"{label} query {q}: an empty query with best {fan.best[q]}"
            continue
        for c in range(Cn):
            want = fan_class(int(fan.cand_feasible[q, c]), int(fan.cand_clamped[q, c]), int(fan.cand_merge_node[q, c]))
            assert int(fan.cand_class[q, c]) == want, f"{label} query {q}: class of candidate {c} is {fan.cand_class[q, c]}, in words {want}"
        keys = [(int(fan.cand_class[q, c]), math.isnan(float(fan.cand_t_end[q, c])), c) for c in range(Cn)]
        best = 0
        for c in range(1, Cn):
            if keys[c][:2] < keys[best][:2] or (keys[c][:2] == keys[best][:2] and float(fan.cand_t_end[q, c]) < float(fan.cand_t_end[q, best])):
                best = c
        assert int(fan.best[q]) == best, f"{label} query {q}: best {fan.best[q]}, the scan gives {best}"
    win = np.maximum(fan.best, 0)
    Dwin = L[np.arange(Q), win]
    done = check_recover(fan, rows, h, closed, lo, hi, nx, ny, P, cfg, Dwin, dir_xy, row, dt, m_cap, k_cap, tally, qs, label=f"{label} winner")
    for q in qs:
        if ok[q]:
            one, K = singles[int(win[q])], int(fan.end_node[q])
            for f in ("node_o", "node_k", "node_t", "node_v", "node_c"):
                assert np.array_equal(bits(getattr(fan, f)[q, :K + 1]), bits(getattr(one, f)[q, :K + 1])), f"{label} query {q}: the winner's {f}"
    return done
