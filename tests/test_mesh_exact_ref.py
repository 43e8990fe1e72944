"""The conditions tests/test_mesh_exact_gpu.py relies on, computed on the CPU from the restatement (tests/ref_mesh.py) on
tests/mesh_exact_scenes.py's scene: every threshold rule of the mesh stage is met EXACTLY, and often - rows at a.y, b.y and
c.y, x_c at 0 and 1, margins of exactly EPSILON and one step to either side, horizontal and vertical edges, projections at
.5, cells with two depths within EPSILON, tracks on the range edge -, the scene tells each rule from its neighbour (a
patched restatement gives other flags, cells or tracks), and three of its polygons are worked by hand.

x_c is not among what ref_mesh.walk yields, so the census takes the rows' ends from `scalar_rows`, a statement-by-statement
transcription of update_scanline like test_mesh_ref.scalar_walk; its pixels must be the walk's, which pins the vectorised
walk on every polygon of the scene by something other than itself."""
import functools
import math

import numpy as np
import pytest

import mesh_exact_scenes as mx
import ref_mesh
from test_mesh_ref import scalar_walk

EPS = mx.EPS
PAIRS = [(i, j) for i in range(3) for j in range(3) if i != j]
AT_LEAST = 10


def scalar_rows(pts, max_x, max_y):
    """ProjectedPolygon::new and update_scanline (output.rs:115-223) for ONE polygon -> per row that is not skipped
    (y, start_x, end_x, x0, x1), a, b, c."""
    def clamp(v, hi):
        c = 0.0 if v < 0.0 else (float(hi) if v > float(hi) else v)
        return 0 if math.isnan(c) else int(c)

    def div(a, b):
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))

    def mix(p, q, k):
        with np.errstate(all="ignore"):
            return float(np.float64(p) * np.float64(1.0 - k) + np.float64(q) * np.float64(k))

    def floor(v):
        return math.floor(v) if math.isfinite(v) else v

    def ceil(v):
        return math.ceil(v) if math.isfinite(v) else v

    key = [int(ref_mesh.total_key(np.array([p[1]]))[0]) for p in pts]
    a, b, c = (pts[i] for i in sorted(range(3), key=lambda i: key[i]))  # (sorted is stable)
    rows = []
    for yi in range(clamp(floor(a[1]), max_y), clamp(ceil(c[1] + 1.0), max_y)):
        y = float(yi)
        if y < a[1] or y > c[1]:
            continue
        if y < b[1] or abs(div(b[1] - c[1], b[0] - c[0])) < EPS:
            sx = mix(a[0], b[0], div(y - a[1], b[1] - a[1]))
        else:
            sx = mix(b[0], c[0], div(y - b[1], c[1] - b[1]))
        ex = mix(a[0], c[0], div(y - a[1], c[1] - a[1]))
        if not sx < ex:
            sx, ex = ex, sx
        rows.append((yi, sx, ex, clamp(floor(sx), max_x), clamp(ceil(ex + 1.0), max_x)))
    return rows, a, b, c


@functools.lru_cache(maxsize=None)
def census(i, j):
    """The culling of camera i's polygons in camera j -> dict of counts (and the emitted pixels, buffer and margins)."""
    s = mx.scene()
    sf = s.surface
    polys = mx.polygons(i).astype(np.int64)
    buf = ref_mesh.depth_buffer(sf, j)
    h, w = buf.shape
    mask, x, y, d = ref_mesh.selected(sf, j)
    pts = ref_mesh.polygon_points(sf, j, polys, x, y, d)
    em = [np.concatenate(q) for q in zip(*ref_mesh.walk(pts, w, h))]
    p, xs, ys, value = em
    with np.errstate(invalid="ignore"):
        margin = buf[ys, xs] - value
    t = ref_mesh.sort_vertices(pts)
    rows = {k: len({(int(a), int(b)) for a, b in zip(p[ys == t[p, k, 1]], ys[ys == t[p, k, 1]])}) for k in range(3)}
    # x_c of every pixel of every row, from the scalar transcription; its emitted pixels are the walk's
    xc0 = xc1 = 0
    mine = []
    for k, tri in enumerate(pts):
        for yi, sx, ex, x0, x1 in scalar_rows([list(v) for v in tri], w, h)[0]:
            if x1 <= x0:
                continue
            cols = np.arange(x0, x1)
            with np.errstate(all="ignore"):
                xc = (cols.astype(np.float64) - sx) / np.float64(ex - sx)
                ok = (0.0 <= xc) & (xc <= 1.0)
            xc0, xc1 = xc0 + int((xc == 0.0).sum()), xc1 + int((xc == 1.0).sum())
            mine += [(k, int(c), yi) for c in cols[ok]]
    assert sorted(mine) == sorted(zip(p.tolist(), xs.tolist(), ys.tolist()))
    # cells that receive two different depths at most EPSILON apart
    cell = ref_mesh.as_usize(ref_mesh.rust_round(y[mask])) * w + ref_mesh.as_usize(ref_mesh.rust_round(x[mask]))
    order = np.lexsort((d[mask], cell))
    c_s, d_s = cell[order], d[mask][order]
    close = (c_s[1:] == c_s[:-1]) & (d_s[1:] != d_s[:-1]) & (d_s[1:] - d_s[:-1] <= EPS)
    both_zeros = (c_s[1:] == c_s[:-1]) & (d_s[1:] == 0.0) & (d_s[:-1] == 0.0) & (np.signbit(d_s[1:]) != np.signbit(d_s[:-1]))
    half = (np.abs(x[mask] - np.trunc(x[mask])) == 0.5) | (np.abs(y[mask] - np.trunc(y[mask])) == 0.5)
    counts = {
        "rows at a.y": rows[0], "rows at b.y": rows[1], "rows at c.y": rows[2],
        "pixels x_c == 0": xc0, "pixels x_c == 1": xc1,
        "margin == EPS": int((margin == EPS).sum()), "margin in (EPS, 2 EPS]": int(((margin > EPS) & (margin <= 2 * EPS)).sum()),
        "margin in (0, EPS)": int(((margin > 0.0) & (margin < EPS)).sum()),
        "polygons a.y == b.y": int((t[:, 0, 1] == t[:, 1, 1]).sum()), "polygons b.y == c.y": int((t[:, 1, 1] == t[:, 2, 1]).sum()),
        "polygons b.x == c.x": int((t[:, 1, 0] == t[:, 2, 0]).sum()),
        "tracks at k + 0.5": int(half.sum()), "cells with two depths within EPS": len(set(c_s[1:][close].tolist())),
    }
    return {"counts": counts, "zeros": int(both_zeros.sum()), "buffer": buf, "pixels": em, "margin": margin, "polygons": polys}


@pytest.mark.parametrize("i,j", PAIRS)
def test_every_rule_is_met_exactly(i, j):
    c = census(i, j)
    h, w = c["buffer"].shape
    keep = ~ref_mesh.obstructs(mx.scene().surface, j, c["polygons"])
    print(f"camera {i}'s {len(c['polygons'])} polygons in camera {j} ({w} x {h} cells, {int(keep.sum())} do not obstruct): "
          + ", ".join(f"{k} {v}" for k, v in c["counts"].items()))
    for name, count in c["counts"].items():
        assert count >= AT_LEAST, (name, count)
    # more than a quarter of the polygons obstruct and more than a quarter do not
    assert 0.25 < keep.mean() < 0.75
    assert w <= 181 and h <= 109 and w > 128
    # no cell holds +0.0 and -0.0 (where the device's key order and np.minimum.at may give different bits), no depth is 0
    assert c["zeros"] == 0 and not (c["buffer"] == 0.0).any()


@pytest.mark.parametrize("i", range(3))
def test_near_threshold_is_not_empty(i):
    s = mx.scene()
    near = ref_mesh.near_threshold(s.surface, mx.polygons(i), camera_i=i, project_to_image=i)
    print(f"camera {i}: near_threshold lists {len(near.polygons)} polygons, {len(near.cells)} cells, {len(near.tracks)} tracks")
    assert near.polygons and near.cells and near.tracks


def test_range_edge_tracks_are_selected_half_open():
    """On lo: in; on hi: out; a quarter below lo: out; a quarter below hi: in - on both axes, in every camera; the image is
    not square, so the two axes have different edges."""
    s = mx.scene()
    for j in range(3):
        mask, x, y, _ = ref_mesh.selected(s.surface, j)
        for want, tr in s.edge[j]["x"].items():
            assert x[tr] == want and mask[tr] == (want in (-140.0, 179.75)), (j, want)
        for want, tr in s.edge[j]["y"].items():
            assert y[tr] == want and mask[tr] == (want in (-84.0, 107.75)), (j, want)
        # -0.0 reaches the sort: a y of -0.0 in the cameras whose second row is e2
        ys = y[s.neg_zero]
        assert (np.signbit(ys) & (ys == 0.0)).sum() >= (3 if j != 1 else 0)


def results():
    """Everything the GPU test compares, from the restatement: per camera the selected tracks, the buffer, and per
    camera_i the flags."""
    s = mx.scene()
    out = {}
    for j in range(3):
        out["points", j] = ref_mesh.camera_points(s.surface, j)[0]
        out["buffer", j] = ref_mesh.depth_buffer(s.surface, j)
        out["flags", j] = ref_mesh.cull(s.surface, j, mx.polygons(j))[0]
    return out


def differs(a, b):
    return a.shape != b.shape or not np.array_equal(a, b, equal_nan=True)


def swapped_img_range(real):
    def img_range(size):
        lo, hi = real(size)
        return lo[::-1], hi[::-1]
    return img_range


ref_mesh_total_key = ref_mesh.total_key


def zero_blind_key(y):
    """total_cmp's key, but -0.0 and +0.0 get the same key (what a plain `<` sort does with them)"""
    return ref_mesh_total_key(np.where(np.asarray(y) == 0.0, 0.0, y))


# name, attribute, its replacement, and what must change - the rule's own output: camera 2's flags, which are decided in
# cameras 0 and 1, for EPSILON (in camera 2 |w| < EPSILON would change the projections as well); flags for the sort
PATCHES = [("EPS = 0", "EPS", 0.0, ("flags", 2)), ("EPS doubled", "EPS", 2 * EPS, ("flags", 2)),
           ("half to even", "rust_round", np.round, ("buffer",)), ("-0.0 == +0.0 in the sort", "total_key", zero_blind_key, ("flags",)),
           ("x and y swapped in img_range", "img_range", swapped_img_range(ref_mesh.img_range), ("points",))]


@pytest.mark.parametrize("name,attr,value,what", PATCHES, ids=[p[0] for p in PATCHES])
def test_scene_tells_a_rule_from_its_neighbour(monkeypatch, name, attr, value, what):
    for i in range(3):
        mx.polygons(i)  # (chosen with the rules as they are)
    before = results()
    monkeypatch.setattr(ref_mesh, attr, value)
    after = results()
    changed = {k for k in before if differs(before[k], after[k])}
    print(f"{name}: changes {sorted(changed)}")
    assert any(k[:len(what)] == what for k in changed), (name, changed)


def hand_case(name, j):
    """-> (the polygon's emitted pixels in camera j, sorted, its flag there, the buffer)"""
    s = mx.scene()
    poly = np.array([s.hand[name]], dtype=np.int64)
    buf = ref_mesh.depth_buffer(s.surface, j)
    x, y = s.surface.project(j)
    pts = ref_mesh.polygon_points(s.surface, j, poly, x, y, s.surface.depth(j))
    h, w = buf.shape
    got = sorted((int(a), int(b), float(v)) for _, xs, ys, vs in ref_mesh.walk(pts, w, h) for a, b, v in zip(xs, ys, vs))
    assert got == [e[1:] for e in scalar_walk([list(v) for v in pts[0]], w, h)]
    return got, bool(ref_mesh.obstructs(s.surface, j, poly)[0]), buf


def test_flat_topped_polygon_by_hand():
    """(10, 2, 1), (12, 2, 1), (10, 4, 1.5) in camera 0: a = (10, 2), b = (12, 2) (equal y: the input order), c = (10, 4);
    rows 2, 3, 4.  Row 2 is not above b.y and the b-c edge is not flat: start from b-c at k = 0 (x = 12), end from a-c at
    k = 0 (x = 10), swapped: x = 10 (x_c = 0), 11, 12 (x_c = 1), all at depth 1.  Row 3: b-c at k = .5 gives x = 11, depth
    1.25; a-c gives x = 10, depth 1.25: x = 10 (x_c = 0) and 11 (x_c = 1).  Row 4: both edges give x = 10: 0 / 0, nothing."""
    got, flag, buf = hand_case("flat_top", 0)
    want = [(10, 2, 1.0), (11, 2, 1.0), (12, 2, 1.0), (10, 3, 1.25), (11, 3, 1.25)]
    assert got == sorted(want)
    assert flag == any(buf[y, x] - v > EPS for x, y, v in want)


def test_vertical_edge_polygon_by_hand():
    """a = (20, 1, 1), b = (22, 3, 1.5), c = (22, 5, .75) in camera 0: b.x == c.x, the b-c slope is -inf (not below EPSILON).
    Row 1: both edges at x = 20: nothing.  Row 2 (above b.y): a-b at k = .5: x = 21, depth 1.25; a-c at k = .25: x = 20.5,
    depth .9375; swapped; x = 20 has x_c = -1, x = 21 has x_c = 1: depth 1.25.  Row 3: b-c at k = 0: x = 22, depth 1.5; a-c
    at k = .5: x = 21, depth .875; x = 21 (x_c = 0) and 22 (x_c = 1).  Row 4: b-c at k = .5: x = 22, depth 1.125; a-c at
    k = .75: x = 21.5, depth .8125; x = 21 has x_c = -1, x = 22 has x_c = 1.  Row 5: both edges at x = 22: nothing."""
    got, flag, buf = hand_case("vertical", 0)
    want = [(21, 2, 1.25), (21, 3, 0.875), (22, 3, 1.5), (22, 4, 1.125)]
    assert got == sorted(want)
    assert flag == any(buf[y, x] - v > EPS for x, y, v in want)


def test_polygon_with_an_infinite_vertex_by_hand():
    """In camera 1: a = (10, 2), b = (+inf, 4) (2 X overflows; y and the depth are finite), c = (10, 6), all at depth 1.
    Row 2: a-b at k = 0 is 10 * 1 + inf * 0 = NaN: the end is NaN, its clamp 0: nothing.  Row 3: a-b at k = .5: x = inf; a-c:
    x = 10; swapped: start 10, end inf, columns 10 .. max_x; x_c = (x - 10) / inf = 0: every pixel from 10 to the buffer's
    last column, depth 1 * 1 + 0 * 1 = 1.  Rows 4, 5, 6: not above b.y, but the b-c slope is -2 / inf = -0, below EPSILON:
    still the a-b edge, at k = 1, 1.5, 2: x = 10 (1 - k) + inf k = inf, depth 1: the same pixels."""
    got, flag, buf = hand_case("infinite", 1)
    w = buf.shape[1]
    assert w == 181
    want = [(x, y, 1.0) for y in (3, 4, 5, 6) for x in range(10, w)]
    assert got == sorted(want)
    assert flag == any(buf[y, x] - v > EPS for x, y, v in want) and flag


# ---- img_range per camera and per axis: mesh_exact_scenes.edge_scene -------------------------------------------------------
def _in_range_set(surface, j):
    return ref_mesh.selected(surface, j, need_seen=False)[0]


def test_edge_scene_tracks_sit_on_both_sides_of_every_range_end():
    """Every camera of edge_scene has w != h and its own dims; its hand-placed tracks project exactly onto lo (in), a
    quarter below lo (out), a quarter below hi (in) and hi (out) of its own img_range, on each axis."""
    s = mx.edge_scene()
    assert len(set(s.image_dims)) == 3 and all(w != h for w, h in s.image_dims)
    assert any(w > h for w, h in s.image_dims) and any(w < h for w, h in s.image_dims)
    for j, size in enumerate(s.image_dims):
        lo, hi = ref_mesh.img_range(size)
        mask, x, y, _ = ref_mesh.selected(s.surface, j)
        for axis, name, got in ((0, "x", x), (1, "y", y)):
            values = list(s.edge[j][name])
            assert values == [lo[axis], lo[axis] - 0.25, hi[axis] - 0.25, hi[axis]]
            for want, tr in s.edge[j][name].items():
                assert got[tr] == want and mask[tr] == (want in (lo[axis], hi[axis] - 0.25)), (j, name, want)


def test_edge_scene_tells_width_from_height_and_camera_from_camera():
    """The restatement with every camera's dims transposed selects another set of tracks in every camera, and in each
    camera one hand-placed track of the x axis AND one of the y axis changes sides: x held against the height's range,
    or y against the width's, is visible there.  So do camera 0's dims used for every camera (cameras 1 and 2), and the
    restatement with img_range's lo and hi exchanged between the axes."""
    s = mx.edge_scene()
    sf = s.surface
    transposed = mx.surface(sf.points, sf.tracks, [(h, w) for w, h in s.image_dims])
    first = mx.surface(sf.points, sf.tracks, [s.image_dims[0]] * 3)
    for j in range(3):
        real, other = _in_range_set(sf, j), _in_range_set(transposed, j)
        assert not np.array_equal(real, other), j
        for name in ("x", "y"):
            tr = list(s.edge[j][name].values())
            assert (real[tr] != other[tr]).any(), (j, name)
        assert not np.array_equal(ref_mesh.camera_points(sf, j)[0], ref_mesh.camera_points(transposed, j)[0])
        if j:
            assert not np.array_equal(real, _in_range_set(first, j)), j


def test_edge_scene_buffers_reach_the_range_ends():
    """The in-range edge tracks stretch every camera's buffer to its own range: ceil(hi - 0.25) + 1 cells per axis, which
    differ between the axes and between the cameras; the polygons of edge_polygons both obstruct and do not."""
    s = mx.edge_scene()
    shapes = []
    for j, size in enumerate(s.image_dims):
        lo, hi = ref_mesh.img_range(size)
        buf = ref_mesh.depth_buffer(s.surface, j)
        assert buf.shape == (int(hi[1]) + 1, int(hi[0]) + 1)
        shapes.append(buf.shape)
    assert len(set(shapes)) == 3 and all(h != w for h, w in shapes)
    for i in range(3):
        keep, _ = ref_mesh.cull(s.surface, i, mx.edge_polygons(i))
        assert 0 < keep.sum() < len(keep), (i, keep)
