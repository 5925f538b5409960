"""The built corridor cases (corridor_cases.py) witness every class of the census, and the census
computes what the oracle computes.  No GPU: the oracle is the C restatement on the CPU.

entry_stream against the library: no public entry point returns a ring's padded entry count M
(RingHost stays inside librl.so), so the layout cases assert M against entry_stream alone here;
a wrong restatement shows on the GPU as a missing layout witness or a differing corridor
(test_gpu_corridor_cases.py), not as a false pass.

Census against the oracle, measured over all kept variants: 0 ulp (lo and hi are bit-equal,
zero signs included; numpy's hypot is the C library's), so the bound stays at the 4 ulp the
expressions allow.
"""
import json
import os

import numpy as np
import pytest

import corridor_cases as K
import oracle_lib as O

RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "corridor_anchor", "census.json")

# the variants whose witness does not survive, and why
DROPPED = {
    # the built samples lie at indices 80 .. 392: every cut ends before the last of them
    "bands_far": ["#N1", "#N2", "#N3", "#N63", "#N65", "#N129", "#N257"],
    "bands_near": ["#N1", "#N2", "#N3", "#N63", "#N65", "#N129", "#N257"],
    # |den| = 2^-53 and 2^-46 are absolute thresholds: beside 2^17 no vertex pair is that close, and
    # scaled by 2^-6 the accepted 2^-46 falls below 1e-15; the cuts end before sample 34
    "thresholds": ["@shift", "@down64", "#N1", "#N2", "#N3"],
    # Rv = 2e5 there, and MISS_NO_CANDIDATE asks for 1e-3 (1 + Rv) = 200 m beside every ray line
    "overrun": ["@shift"],
    # the first gap starts at sample 16
    "gaps": ["#N1", "#N2", "#N3"],
    "outlier": ["#N1", "#N2", "#N3"],
}


@pytest.fixture(scope="module")
def variants():
    return K.variants()


def test_no_base_case_is_dropped_and_the_dropped_table_holds(variants):
    kept, dropped = variants
    assert sorted(dropped) == sorted(n + s for n, ss in DROPPED.items() for s in ss)
    ids = {v[0] for v in kept}
    for case in K.base_cases():
        assert f"{case.name}@base" in ids, case.name


def test_every_class_is_witnessed(variants):
    kept, _ = variants
    total = {c: np.zeros((2, 2), dtype=np.int64) for c in K.CLASSES}
    for vid, case, fr, prob, cfg, cen in kept:
        for c, v in cen.counts().items():
            total[c] += np.array(v)
    for c, t in total.items():
        assert t.sum() >= 8, (c, t.tolist())
        assert (t.sum(axis=1) > 0).all(), f"{c}: a ring has no witness {t.tolist()}"
        assert (t.sum(axis=0) > 0).all(), f"{c}: a direction has no witness {t.tolist()}"


def test_every_case_holds_its_classes(variants):
    kept, _ = variants
    for vid, case, fr, prob, cfg, cen in kept:
        for c in case.expect:
            assert cen.count(c) > 0, (vid, c)


def test_layout_classes_on_each_ring(variants):
    kept, _ = variants
    for vid, case, fr, prob, cfg, cen in kept:
        if case.M is not None:
            got = tuple(K.entry_stream(s)[2] for s in (prob.inner_seg, prob.outer_seg))
            assert got == case.M, (vid, got, case.M)
        for k in case.layouts:
            for r in (K.INNER, K.OUTER):
                assert cen.layout[r][k] > 0, (vid, k, r)
    for k in K.LAYOUTS:
        for r in (K.INNER, K.OUTER):
            assert sum(v[5].layout[r][k] for v in kept if v[1].name.startswith("decoy")) > 0, (k, r)


def test_entry_stream_places_the_decoy_layouts():
    for name, (na, nd, first_end) in K.DECOY_LAYOUTS.items():
        case = K.decoys(name)
        for seg in (case.prob.inner_seg, case.prob.outer_seg):
            end_idx, dummy, M = K.entry_stream(seg)
            e = int(np.flatnonzero(seg[:, 0] == -1.0)[0])          # the real chain's first segment
            assert end_idx[e] == first_end and dummy[e] and M == 64, (name, end_idx[e], M)
            # the entries of the block(s) before it, but for the last, belong to the decoys
            blk = [j for j in range(len(seg)) if first_end - 1 - nd <= end_idx[j] < first_end]
            assert blk and all(seg[j, 0] <= -500.0 for j in blk), (name, blk)


def test_tolerance_cases_have_their_class(variants):
    kept, _ = variants
    n = 0
    for vid, case, fr, prob, cfg, cen in kept:
        for i, r, d, c, want in case.direct:
            assert K.holds(cen, i, r, d, c, want), f"{vid}: sample {i}, ring {r}, direction {d}: {c} != {want}"
            n += 1
    assert n >= 100


def test_census_equals_the_oracle(variants):
    kept, _ = variants
    worst = 0.0
    for vid, case, fr, prob, cfg, cen in kept:
        olo, ohi = O.run_oracle_corridor(prob, cfg)
        guard = prob.veh_width * 0.5 + cfg.safety_margin_m
        for what, g, r in (("lo", cen.lo, olo), ("hi", cen.hi, ohi)):
            assert ((g == 0) == (r == 0)).all() and (np.signbit(g) == np.signbit(r)).all(), (vid, what)
            ulp = np.abs(g - r) / np.spacing(np.maximum(np.abs(r), guard))
            worst = max(worst, float(ulp.max()))
            assert ulp.max() <= 4, (vid, what, float(ulp.max()), int(np.argmax(ulp)))
    print(f"census against the oracle: worst {worst} ulp over {len(kept)} variants")


def test_record_is_current(variants):
    """profiles/corridor_anchor/census.json (python tests/corridor_cases.py) holds this census."""
    with open(RECORD) as f:
        rec = json.load(f)
    kept, dropped = variants
    assert rec["dropped"] == dropped
    assert sorted(rec["new"]) == sorted(v[0] for v in kept)
    for vid, case, fr, prob, cfg, cen in kept:
        if case.name == "spokes":       # built with cos and sin: a libm may move a chain start across its ray line
            continue
        assert rec["new"][vid] =={c: v for c, v in cen.counts().items() if np.sum(v)}, vid
    # what the older cases never reached
    assert np.sum(rec["old_total"]["MISS_NO_CANDIDATE"]) == 0 and np.sum(rec["old_total"]["ON_RING"]) == 0


def test_classes_survive_the_first_outer_iteration(variants):
    """The optimisers cast their second corridor about a moved path.  Every base case still holds
    its classes about the oracle's seed-0 path after one outer iteration (none keeps its witness
    at the centre line only)."""
    kept, _ = variants
    for vid, case, fr, prob, cfg, cen in kept:
        if vid.endswith("@base"):
            cm = K.census(K.moved_problem(prob, cfg), cfg)
            for c in case.expect:
                assert cm.count(c) > 0, (vid, c)
