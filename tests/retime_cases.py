"""What tests/test_retime_vpass_cpu.py and tests/test_gpu_retime_vpass.py share (no tests here): the
rows on which the retime stage must reproduce the oracle's v-pass bit for bit (DESIGN §3p "Anchored
to the oracle"), and the check itself.  A plain helper module like vpass_anchor_cases, whose rows,
oracle call and bit view it reuses: no fixtures, no pytest settings.

The rows are open and straight (x = i h, y = heading = ax = 0) with a curvature column of their
own and the speed column r = +inf, so that the row's speed never caps and the stage's nodes are
the row's samples (the pose is sample 0: segment 0, u = 0, d_0 = h).  Then the stage's ceiling is
the oracle's initial profile (max_vpass_iters = 0) and its march the oracle's converged one:

    rows: vpass_anchor_cases' wave, flat and tight_h02, and scurve, kappa = 0.08 sin(2 pi i / 60) at
        h = 0.5: corner after corner, each braking for the next;
    corner: kappa[N - 1] = -3;  slow start: kappa[0] = 40;
    v0 = the oracle's converged v[0];  K_cap = N - 1, so that node K is the last sample.
"""
from __future__ import annotations

import collections
import functools
import itertools

import numpy as np

import cfg_cases
import vpass_anchor_cases as VA
from vpass_anchor_cases import N, bits

ITERS = 12                              # sweeps of the converged oracle runs (asserted to settle earlier)
ROWS = {**VA.ROWS, "scurve": ("scurve", 0.5)}
NAMES = tuple(ROWS)
B = len(ROWS)
CASES = list(cfg_cases.CASES)
FLAGS = list(itertools.product((False, True), (False, True)))        # (corner, slow_start)
KW = dict(dt=0.05, m_cap=8, k_cap=N - 1)


def kappa(name: str, corner: bool, slow_start: bool) -> np.ndarray:
    if name != "scurve":
        return VA.kappa(name, corner, slow_start)
    k = 0.08 * np.sin(2.0 * np.pi * np.arange(N) / 60.0)
    if corner:
        k[N - 1] = VA.KAPPA_CORNER
    if slow_start:
        k[0] = VA.KAPPA_START
    return k


Anchor = collections.namedtuple("Anchor", "names rows h poses row v0 kappa want_c want sweeps")


@functools.lru_cache(maxsize=None)
def anchor(case: str, corner: bool, slow_start: bool) -> Anchor:
    """The B rows of one call under a case's cfg, one query per row, read-only: rows (the six
    [B, N] arrays, the speed column +inf), h [B], poses [B, 2], row [B], v0 [B]; want_c [B, N] the
    oracle's initial profile, want [B, N] its converged one, sweeps: the sweeps the B runs took."""
    cfg = cfg_cases.case_cfg(case)
    h = np.array([ROWS[n][1] for n in NAMES])
    kap = np.stack([kappa(n, corner, slow_start) for n in NAMES])
    want_c, want, sweeps = np.zeros((B, N)), np.zeros((B, N)), []
    for b in range(B):
        want_c[b], _ = VA.oracle_v(cfg, kap[b], h[b], 0)
        want[b], s = VA.oracle_v(cfg, kap[b], h[b], ITERS)
        sweeps.append(s)
    z = np.zeros((B, N))
    rows = (np.arange(N)[None, :] * h[:, None], z, z, kap, np.full((B, N), np.inf), z)
    out = Anchor(NAMES, rows, h, np.zeros((B, 2)), np.arange(B, dtype=np.int32), want[:, 0].copy(), kap, want_c, want,
                 tuple(sweeps))
    for a in rows + (h, out.poses, out.row, out.v0, want_c, want):
        a.setflags(write=False)
    return out


def check(got, a: Anchor, case: str, slow_start: bool, label: str) -> None:
    """A Retime answer of the anchor's queries against the oracle, bit for bit: node_c is the
    initial profile, node_v the converged one, and without the slow start node_b as well at every
    node at which the march runs on the envelope: the whole row unless the row asks for
    acceleration."""
    K = N - 1
    msg = f"{label} {case}"
    np.testing.assert_array_equal(got.seg, 0, err_msg=msg)
    np.testing.assert_array_equal(bits(got.u), bits(np.zeros(B)), err_msg=msg)
    np.testing.assert_array_equal(got.end_node, K, err_msg=msg)
    np.testing.assert_array_equal(got.feasible, 1, err_msg=msg)
    np.testing.assert_array_equal(got.overspeed, 0, err_msg=msg)
    assert got.node_v.shape == (B, N)
    assert max(a.sweeps) < ITERS, f"{case}: the oracle has not converged in {ITERS} sweeps: {a.sweeps}"
    for b, name in enumerate(a.names):
        np.testing.assert_array_equal(bits(got.node_c[b]), bits(a.want_c[b]), err_msg=f"{msg} {name}: node_c vs the oracle's initial v")
        np.testing.assert_array_equal(bits(got.node_v[b]), bits(a.want[b]), err_msg=f"{msg} {name}: node_v vs the oracle's v")
        # the envelope is never below the march of a feasible start
        assert np.all(got.node_b[b] >= got.node_v[b]), f"{msg} {name}: node_b < node_v"
        if not slow_start:
            # where the march runs on the envelope, the envelope is the oracle's profile; that is
            # the whole row wherever the oracle's initial profile never rises, since no node then
            # asks for acceleration (the scurve row, and the wave under vcap_huge, rise: there the
            # car accelerates out of a corner below the envelope, as the oracle's profile does)
            on = bits(got.node_v[b]) == bits(got.node_b[b])
            if np.all(np.diff(a.want_c[b]) <= 0.0):
                assert np.all(on), f"{msg} {name}: node_v vs node_b on a row whose ceiling never rises"
            assert on[0] and np.count_nonzero(on) >= 10, f"{msg} {name}: {np.count_nonzero(on)} nodes on the envelope"
            np.testing.assert_array_equal(bits(got.node_b[b][on]), bits(a.want[b][on]), err_msg=f"{msg} {name}: node_b vs the oracle's v")
