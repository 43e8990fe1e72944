"""Scenes and the host restatement of the cross-check for tests/test_fused_finish_gpu.py (cvhip_ctx_set_fused_finish: the
last level's forward filter inside complete()'s expansion).

The restatement works on the UNFILTERED full-resolution grids of both directions, ([h, w, 2] int32 match positions, -1 =
None), and states cross_check_filter / cross_check_point (mod.rs:552-624) at scale 1 in numpy: a forward match (mx, my) of
cell (x, y) stays when some reverse cell within +-4 of (mx, my) holds a match within +-4 of (x, y).  census() counts what a
scene must contain for the fused kernel's paths to be exercised at all."""
import numpy as np

import cases
from cybervision_amd import synth

SEARCH_AREA = 4  # CROSS_CHECK_SEARCH_AREA at scale 1
SCENES = ["tilt3_200x150", "ragged_dims_occluded", "sem320x200", "clusters_192x136"]


def make_scene(name):
    if name == "ragged_dims_occluded":
        # tests/cases.py's ragged_dims (w1 != w2, h1 != h2) gives the filter 16 cells to remove: here image 2 also has a strip
        # that image 1 does not see and a patch displaced against its surroundings
        c = dict(cases.make_case("ragged_dims"), name=name)
        b = c["img2"].copy()
        other = synth.make_pair(b.shape[1], b.shape[0], seed=58)[0]
        b[:, 60:72] = other[:, 60:72]
        b[90:140, 110:160] = np.roll(b, 6, axis=1)[90:140, 110:160]
        c["img2"] = np.ascontiguousarray(b)
        return c
    if name != "clusters_192x136":
        return cases.make_case(name)
    # 192 x 136 (three 64-cell segments per row, 136 = 34 x 4 rows) against a wider and taller second image.  Image 2 has a
    # strip that image 1 does not see (an occluder: unrelated texture) and a patch that moves against its surroundings,
    # so that the filter removes cells in clusters; small unrelated blocks sit at all four borders.
    w, h = 192, 136
    a, b0, _ = synth.make_pair(w, h, seed=31)
    b = np.ascontiguousarray(np.pad(b0, ((0, 9), (0, 13)), mode="edge"))
    other = synth.make_pair(b.shape[1], b.shape[0], seed=57)[0]
    b[:, 84:99] = other[:, 84:99]                       # the occluded strip
    b[40:80, 120:170] = np.roll(b, 7, axis=1)[40:80, 120:170]  # displaced against the field around it
    for ys, xs in ((slice(0, 10), slice(20, 60)), (slice(h - 9, h + 9), slice(100, 150)), (slice(50, 100), slice(0, 9)),
                   (slice(15, 50), slice(w - 10, w + 13))):
        b[ys, xs] = other[ys, xs]
    steps = synth.optimal_scale_steps(w, h)
    return dict(name=name, img1=a, img2=b, F=np.asarray(synth.f_tilt(1.0), dtype=np.float64), projection=0, steps=steps)


def unfiltered_last_level(oracle, c):
    """The oracle's grids after the two search passes of scale 1 and before either cross-check:
    (forward xy, reverse xy), and the forward grid (xy, corr) after the level's filters."""
    p1, p2 = cases.pyramids(c)
    h1, w1 = c["img1"].shape
    h2, w2 = c["img2"].shape
    oc = oracle.Corr((w1, h1), (w2, h2), c["F"], c["projection"], 8)
    try:
        for i in range(c["steps"]):
            k = c["steps"] - i
            oc.correlate_images(p1[k], p2[k], 1.0 / float(1 << k))
        oc.step(p1[0], p2[0], 1.0, 0)
        oc.step(p2[0], p1[0], 1.0, 1)
        fwd, rev = oc.get(0)[0].copy(), oc.get(1)[0].copy()
        oc.cross_check(1.0, 0)
        oc.cross_check(1.0, 1)
        return fwd, rev, oc.get(0), oc.get(1)
    finally:
        oc.close()


def restate_filter(own, other):
    """-> (probe_ok, supported): per cell of `own`, whether the other grid's cell at the match points back, and whether any
    cell of the (2 * 4 + 1)^2 window around it does.  False where the cell is None."""
    h, w = own.shape[:2]
    rh, rw = other.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    some = own[..., 0] >= 0
    mx, my = own[..., 0], own[..., 1]
    sa = SEARCH_AREA

    def back(dx, dy):
        px, py = mx + dx, my + dy
        ok = some & (px >= 0) & (px < rw) & (py >= 0) & (py < rh)
        r = other[np.where(ok, py, 0), np.where(ok, px, 0)]
        return ok & (r[..., 0] >= 0) & (np.abs(r[..., 0] - xs) <= sa) & (np.abs(r[..., 1] - ys) <= sa)

    probe_ok = back(0, 0)
    supported = probe_ok.copy()
    for dy in range(-sa, sa + 1):
        for dx in range(-sa, sa + 1):
            supported |= back(dx, dy)
    return probe_ok, supported


def census(own, other):
    """What the scene gives the filter to do (forward direction)."""
    h, w = own.shape[:2]
    some = own[..., 0] >= 0
    probe_ok, supported = restate_filter(own, other)
    failing = some & ~probe_ok
    odd_segments = 0
    for x0 in range(0, w, 64):
        n = failing[:, x0:x0 + 64].sum(axis=1)
        odd_segments += int(((n >= 3) & (n % 2 == 1)).sum())
    b = SEARCH_AREA
    return dict(removed=int((some & ~supported).sum()), rescued=int((failing & supported).sum()), odd_segments=odd_segments,
                top=bool(failing[:b].any()), bottom=bool(failing[h - b:].any()), left=bool(failing[:, :b].any()),
                right=bool(failing[:, w - b:].any()), kept=int(supported.sum()))
