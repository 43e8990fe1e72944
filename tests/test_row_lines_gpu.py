"""GPU parity of the lean box walk's row table (box_body.inc; cvhip_ctx_set_row_lines) on the scenes of
tests/row_line_scenes.py: exactly horizontal lines on and off the pixel's row, at the binades where the stripes' rows are
checked one by one, leaving the image; matrices that are horizontal to within a rounding, where the table must be
refused; and every route that reaches a lean box launch.  test_row_lines.py shows from the oracle's lines that the scenes
are what they are made for."""
import functools

import numpy as np
import pytest

import row_line_scenes as rs
from cybervision_amd import correlation, sharding

pytestmark = pytest.mark.gpu
F, R = correlation.CorrelationDirection.Forward, correlation.CorrelationDirection.Reverse
POISON = 1 << 36  # a counting kernel that disagrees with the table adds 2^44 to `candidates`


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def scene(name):
    return rs.make_scene(name)


_ORACLE = {}


def _oracle_levels(oracle, name):
    c = scene(name)
    p1, p2 = rs.pyramids(c)
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


def oracle_levels(oracle, name):
    """The oracle's two grids after every level and its candidate count - computed once per pair of images and F."""
    key = rs.image_key(name)
    if key not in _ORACLE:
        _ORACLE[key] = _oracle_levels(oracle, name)
    return _ORACLE[key]


def run(dev, name, rows, exact_scores, per_level=False, count=False):
    """-> (grids after every level [(fwd, rev)] or only the last, counters or None, the getter's answer, live result bands)."""
    c = scene(name)
    route = c["route"]
    p1, p2 = rs.pyramids(c)
    h1, w1 = c["img1"].shape
    h2, w2 = c["img2"].shape
    pc = correlation.PointCorrelations(dev, (w1, h1), (w2, h2), c["F"], correlation.ProjectionMode(c["projection"]))
    try:
        pc.set_exact_scores(exact_scores)
        pc.set_row_lines(rows)
        pc.set_box_fold(route.get("fold", True))
        pc.set_profiling(False, count)
        if "band" in route:
            assert pc.set_row_band(*route["band"]), "horizontal lines are row-local"
        if "result_bands" in route:
            pc.set_result_bands(route["result_bands"])
        out = []
        for i in range(c["steps"] + 1):
            k = c["steps"] - i
            pc.correlate_images(p1[k], p2[k], 1.0 / float(1 << k), fused=route.get("fused", True))
            if per_level or k == 0:
                # (an independent band leaves the reverse grid to the context that owns those rows)
                grids = (pc.complete(F),) if "band" in route else (pc.complete(F), pc.complete(R))
                out.append(tuple((xy.copy(), co.copy()) for xy, co in grids))
        live = pc.result_bands() if "result_bands" in route else None
        return out, pc.get_counters() if count else None, pc.get_row_lines_used(), live
    finally:
        pc.close()


def same_grid(got, want, rows, what, scores=True):
    r0, r1 = rows
    assert (got[0][r0:r1] == want[0][r0:r1]).all(), f"{what}: match positions differ"
    if scores:
        valid = want[0][r0:r1, :, 0] >= 0
        assert (bits(got[1])[r0:r1][valid] == bits(want[1])[r0:r1][valid]).all(), f"{what}: score bits differ"


@pytest.mark.parametrize("name", sorted(rs.SCENES))
def test_row_table_matches_oracle_and_per_lane_lines(gpu_device, oracle, name):
    c = scene(name)
    want, cand = oracle_levels(oracle, name)
    band = c["route"].get("band")
    h1 = c["img1"].shape[0]
    # (an independent band computes its rows of the final forward grid; everything else both grids, whole)
    rows_f = sharding.shard_rows(h1, *band) if band else (0, h1)
    # every pass writes the reference's scores, the counting kernels (which evaluate every lane's line beside the table's
    # and poison the count on any difference): both grids, positions and score bits, at every level's hand-over
    got, cnt, used, _ = run(gpu_device, name, True, True, per_level=not band, count=True)
    print(name, "used", used, "counters", cnt, "oracle candidates", cand)
    assert used == c["used"]
    if band:
        same_grid(got[-1][0], want[-1][0], rows_f, f"{name} band {band} forward")
        assert cnt["candidates"] < POISON  # (the band's halo rows are searched too: more candidates than its share)
    else:
        assert len(got) == len(want)
        for lv, (g, w) in enumerate(zip(got, want)):
            for d, what in ((0, "forward"), (1, "reverse")):
                same_grid(g[d], w[d], (0, w[d][0].shape[0]), f"{name} level {lv} {what}")
        assert cnt["candidates"] == cand
    # the default score mode (the benchmark's), the plain kernels: the switch on equals the switch off bit for bit (the NaN
    # cells included), and both are the oracle's forward grid and reverse positions
    (on,), _, used_on, live_on = run(gpu_device, name, True, False)
    (off,), _, used_off, live_off = run(gpu_device, name, False, False)
    assert used_on == c["used"] and used_off == (False, False)
    if "result_bands" in c["route"]:
        assert live_on == live_off == c["route"]["result_bands"]
    same_grid(on[0], want[-1][0], rows_f, f"{name} default scores forward")
    if not band:
        same_grid(on[1], want[-1][1], (0, on[1][0].shape[0]), f"{name} default scores reverse", scores=False)
    for d in ((0,) if band else (0, 1)):
        r0, r1 = rows_f if band else (0, on[d][0].shape[0])
        assert (on[d][0][r0:r1] == off[d][0][r0:r1]).all() and (bits(on[d][1])[r0:r1] == bits(off[d][1])[r0:r1]).all(), \
            f"{name}: the table changes direction {d}"
    # ... and so is the candidate count of the default mode's counting kernels, with the table and without
    _, cnt_on, _, _ = run(gpu_device, name, True, False, count=True)
    _, cnt_off, _, _ = run(gpu_device, name, False, False, count=True)
    assert cnt_on == cnt_off
    if not band:
        assert cnt_on["candidates"] == cand
