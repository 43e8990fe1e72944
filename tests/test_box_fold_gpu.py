"""GPU parity of the lean box walk's fold (box_body.inc) on the scenes of tests/fold_scenes.py: small
rectified pairs whose search ranges drift along the waves one way, the other way, both ways and not at all, with ranges
near the walk's admission limit and with lanes without a pixel inside waves.  test_box_fold.py shows from the oracle's
ranges that the scenes are what they are made for."""
import functools

import numpy as np
import pytest

import fold_scenes as fs
from cybervision_amd import correlation

pytestmark = pytest.mark.gpu
F, R = correlation.CorrelationDirection.Forward, correlation.CorrelationDirection.Reverse

# scene -> (ascending folds, descending folds): True = the counters must show some, False = none
EXPECT = {
    "ramp_up": (True, None), "ramp_down": (None, True), "flat": (False, False), "tent_valley": (True, True),
    "edge": (True, True), "ramp_half": (None, None), "ramp_strip": (None, None),
}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def scene(name):
    return fs.make_scene(name)


@functools.lru_cache(maxsize=None)
def oracle_levels(oracle, name):
    """The oracle's two grids after every level (computed once per scene), and its candidate count."""
    c = scene(name)
    p1, p2 = fs.pyramids(c)
    h1, w1 = c["img1"].shape
    h2, w2 = c["img2"].shape
    oc = oracle.Corr((w1, h1), (w2, h2), c["F"], c["projection"], 8)
    levels = []
    try:
        for i in range(c["steps"] + 1):
            k = c["steps"] - i
            oc.correlate_images(p1[k], p2[k], 1.0 / float(1 << k))
            levels.append(tuple((xy.copy(), co.copy()) for xy, co in (oc.get(0), oc.get(1))))
    finally:
        oc.close()
    _, _, cand = oracle.correlate_dense(p1, p2, c["F"], c["projection"], 8)
    return levels, cand


def run(dev, name, fold, exact_scores, per_level=False, count=True):
    """count: the candidate-counting instantiations of the kernels (profiling) instead of the plain ones.
    -> (grids after every level [(fwd, rev)] or only the last, counters, fold counters)."""
    c = scene(name)
    p1, p2 = fs.pyramids(c)
    h1, w1 = c["img1"].shape
    h2, w2 = c["img2"].shape
    pc = correlation.PointCorrelations(dev, (w1, h1), (w2, h2), c["F"], correlation.ProjectionMode(c["projection"]))
    try:
        pc.set_exact_scores(exact_scores)
        pc.set_box_fold(fold)
        pc.set_profiling(False, count)
        out = []
        for i in range(c["steps"] + 1):
            k = c["steps"] - i
            pc.correlate_images(p1[k], p2[k], 1.0 / float(1 << k))
            if per_level or k == 0:
                out.append(tuple((xy.copy(), co.copy()) for xy, co in (pc.complete(F), pc.complete(R))))
        return out, pc.get_counters() if count else None, pc.get_box_fold_counters() if count else None
    finally:
        pc.close()


@pytest.mark.parametrize("name", sorted(fs.SCENES))
def test_fold_matches_oracle_and_plain_walk(gpu_device, oracle, name):
    want, cand = oracle_levels(oracle, name)
    # every pass writes the reference's scores: both grids, positions and score bits, at every level's hand-over
    got, cnt_x, fold_x = run(gpu_device, name, True, True, per_level=True)
    assert len(got) == len(want)
    for lv, (g, w) in enumerate(zip(got, want)):
        for d, what in ((0, "forward"), (1, "reverse")):
            assert (g[d][0] == w[d][0]).all(), f"{name} level {lv} {what}: match positions differ"
            valid = w[d][0][..., 0] >= 0
            assert (bits(g[d][1])[valid] == bits(w[d][1])[valid]).all(), f"{name} level {lv} {what}: score bits differ"
    assert cnt_x["candidates"] == cand  # no candidate dropped, none visited twice
    # the default score mode (the benchmark's): forward positions and score bits, reverse positions
    (on,), cnt_on, fold_on = run(gpu_device, name, True, False)
    (off,), cnt_off, fold_off = run(gpu_device, name, False, False)
    for g, what in ((on, "fold on"), (off, "fold off")):
        assert (g[0][0] == want[-1][0][0]).all() and (g[1][0] == want[-1][1][0]).all(), f"{name} {what}: positions differ"
        valid = want[-1][0][0][..., 0] >= 0
        assert (bits(g[0][1])[valid] == bits(want[-1][0][1])[valid]).all(), f"{name} {what}: forward score bits differ"
    # fold on and fold off: identical bits (the NaN cells included) and identical work - the same candidates, exact
    # evaluations, pixels with several contenders and pixels handed to the whole-corridor list
    for d in (0, 1):
        assert (on[d][0] == off[d][0]).all() and (bits(on[d][1]) == bits(off[d][1])).all()
    assert cnt_on == cnt_off and cnt_on["candidates"] == cand
    # the plain instantiations (no counting: what a run without profiling launches) give the same bits
    (plain_on,), _, _ = run(gpu_device, name, True, False, count=False)
    (plain_off,), _, _ = run(gpu_device, name, False, False, count=False)
    for d in (0, 1):
        for g in (plain_on, plain_off):
            assert (g[d][0] == on[d][0]).all() and (bits(g[d][1]) == bits(on[d][1])).all(), f"{name}: plain kernels differ"
    # the counters: what the switch does
    print(name, "fold on", fold_on, "off", fold_off, "counters", cnt_on)
    assert fold_x == fold_on
    assert fold_off["union_steps"] == fold_on["union_steps"] == fold_off["folded_steps"]
    assert fold_off["pairs_ascending"] == 0 and fold_off["pairs_descending"] == 0
    assert fold_on["union_steps"] - fold_on["folded_steps"] == fold_on["pairs_ascending"] + fold_on["pairs_descending"]
    asc, desc = EXPECT[name]
    for want_some, key in ((asc, "pairs_ascending"), (desc, "pairs_descending")):
        if want_some is True:
            assert fold_on[key] > 0, f"{name}: {fold_on}"
        elif want_some is False:
            assert fold_on[key] == 0, f"{name}: {fold_on}"
    # ... and they are what the oracle's ranges predict, wave by wave, for the workgroups the lean plan admits
    # (fold_scenes.admitted): the admitted set - and so the declined work list - is the prediction's, with the fold on and off
    pred = fs.scene_folds(oracle, scene(name), only_admitted=True)
    assert (fold_on["union_steps"], fold_on["folded_steps"], fold_on["pairs_ascending"], fold_on["pairs_descending"]) == \
           (pred["union"], pred["folded"], pred["asc"], pred["desc"]), f"{name}: {fold_on} against {pred}"
    if name == "ramp_half":
        # unions near the walk's admission limit: hundreds of waves sit in workgroups that decline, and the others walk and fold
        assert pred["declined"] >= 500 and pred["asc"] + pred["desc"] > 0
