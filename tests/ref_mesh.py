"""CPU restatement (numpy, f64) of the reference's mesh stage - test infrastructure only.

Transcribes, citing zlogic/cybervision v0.20.3 src/output.rs (and src/triangulation.rs where said):
  - Surface::project_point (triangulation.rs:63-74), Camera::point_depth (triangulation.rs:492-495), img_range (:613-624)
  - Mesh::process_camera's camera points (:401-423) and culling loop (:457-508)
  - DepthBuffer::new / polygon_obstructs (:256-353)
  - ProjectedPolygon and its iterator (:107-254), quirks included (division by zero is not special-cased: NaN and
    infinity flow through the comparisons and clamps as in Rust)
  - Polygon::new, Ord, the per-camera sort + dedup and the final sort by camera (:50-105, 384, 510-516)
  - ImageWriter (:1016-1143) without the colour table and the encoder
Every arithmetic operation is one numpy operation in the reference's order (numpy does not fuse).  Vectorised over
polygons, their rows and the pixels of a row (all flattened): no Python loop runs over rows or pixels.

Defined where the reference's result depends on its thread order (par_bridge, sort_unstable): a depth-buffer cell is the
MINIMUM of its depths (an image cell the MAXIMUM) - one of the reference's outcomes unless two depths of a cell differ
by a non-zero amount <= EPSILON -, the camera points come in track order, and a vertex triple that two cameras produce
stays with the LOWEST camera.
Nothing in cybervision_amd/ may import this module.
"""
from __future__ import annotations

import numpy as np

import ref_triangulation as rt

EPS = np.finfo(np.float64).eps
MAX_CENTER_DISTANCE = 4.0  # output.rs:21
TOL = 1e-9


class Surface:
    """triangulation::Surface as the mesh stage reads it: points [n, 3], tracks [n, m, 2] ((-1, -1) = None), cameras
    [rt.Camera], their projections [m, 3, 4] (K [R | t], as the surface holds them) and the images' (width, height)."""

    def __init__(self, points, tracks, cameras, projections, image_dims):
        self.points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        self.tracks = np.ascontiguousarray(tracks, dtype=np.int32)
        self.cameras = list(cameras)
        self.projections = np.ascontiguousarray(projections, dtype=np.float64).reshape(len(self.cameras), 3, 4)
        self.image_dims = [(int(w), int(h)) for w, h in image_dims]

    @staticmethod
    def from_poses(points, tracks, poses, image_dims):
        """cameras given as (K, r, t), r the axis-angle vector: Camera { k, r, t } and its own projection K [matrix_r(r) | t]."""
        cams = [rt.Camera(K, r, t) for K, r, t in poses]
        return Surface(points, tracks, cams, [c.projection() for c in cams], image_dims)

    @staticmethod
    def from_device(surface, image_dims):
        """a cybervision_amd.triangulation.Surface (cameras with r, t, projection; K is not needed here)."""
        cams = [rt.Camera(np.eye(3), c.r, c.t) for c in surface.cameras]
        return Surface(surface.points, surface.tracks, cams, [np.asarray(c.projection).reshape(3, 4) for c in surface.cameras],
                       image_dims)

    def seen(self, j):
        return self.tracks[:, j, 0] >= 0

    def project(self, j):
        """project_point (triangulation.rs:63-74): P (X, Y, Z, 1) summed column by column -> (x [n], y [n])."""
        P, X = self.projections[j], self.points
        p = [((P[k, 0] * X[:, 0] + P[k, 1] * X[:, 1]) + P[k, 2] * X[:, 2]) + P[k, 3] for k in range(3)]
        scale = np.where(np.abs(p[2]) < EPS, 1.0, p[2])
        with np.errstate(all="ignore"):
            return p[0] / scale, p[1] / scale

    def depth(self, j):
        """point_depth (triangulation.rs:492-495): (r_matrix (X + r_matrix^T t)).z, each dot product left to right."""
        R, t, X = self.cameras[j].r_matrix, self.cameras[j].t, self.points
        rtt = [(R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2] for k in range(3)]
        q = [X[:, k] + rtt[k] for k in range(3)]
        return (R[2, 0] * q[0] + R[2, 1] * q[1]) + R[2, 2] * q[2]

    def in_range(self, j, x, y):
        """img_range (:613-624): half-open [c - 4 size, c + 4 size) per axis."""
        lo, hi = img_range(self.image_dims[j])
        with np.errstate(invalid="ignore"):
            return (lo[0] <= x) & (x < hi[0]) & (lo[1] <= y) & (y < hi[1])


def img_range(size):
    lo, hi = [], []
    for s in size:
        s = float(s)
        c = s / 2.0
        lo.append(c - s * MAX_CENTER_DISTANCE)
        hi.append(c + s * MAX_CENTER_DISTANCE)
    return lo, hi


# ---- Rust's conversions ----------------------------------------------------------------------------------------------------
def rust_round(v):
    """f64::round: half away from zero."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        r = np.trunc(v)
        return r + np.sign(v) * (np.abs(v - r) >= 0.5)


def as_usize(v):
    """`as usize`: saturating, NaN -> 0 (as int64, capped at 2^62)."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v) | (v < 0.0), 0.0, np.minimum(v, 2.0 ** 62)).astype(np.int64)


def clamp_usize(v, mx):
    """f64::clamp(0.0, mx as f64) as usize: NaN stays NaN and converts to 0."""
    with np.errstate(invalid="ignore"):
        c = np.where(v < 0.0, 0.0, np.where(v > float(mx), float(mx), v))
    return as_usize(c)


def total_key(y):
    """f64::total_cmp's integer key."""
    b = np.ascontiguousarray(y, dtype=np.float64).view(np.int64)
    return b ^ ((b >> 63) & np.int64(0x7FFFFFFFFFFFFFFF))


def _near_int(v):
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & (np.abs(v - np.round(v)) <= TOL)


def _near_half(v):
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & (np.abs(np.abs(v - np.trunc(v)) - 0.5) <= TOL)


class Near:
    """What near_threshold collects: polygon indices, cells (camera, y, x) and tracks whose deciding quantity lies within
    TOL of its threshold."""

    def __init__(self):
        self.polygons, self.cells, self.tracks = set(), set(), set()

    def empty(self):
        return not (self.polygons or self.cells or self.tracks)


# ---- camera points, depth buffer ----------------------------------------------------------------------------------------------
def selected(surface, j, need_seen=True, near=None):
    """-> (mask [n], x, y, depth): the tracks (with a point in camera j, if need_seen) whose projection is in range."""
    x, y = surface.project(j)
    mask = surface.in_range(j, x, y)
    if need_seen:
        mask = mask & surface.seen(j)
    if near is not None:
        lo, hi = img_range(surface.image_dims[j])
        with np.errstate(invalid="ignore"):
            edge = (np.abs(x - lo[0]) <= TOL) | (np.abs(x - hi[0]) <= TOL) | (np.abs(y - lo[1]) <= TOL) | (np.abs(y - hi[1]) <= TOL)
        near.tracks.update(np.nonzero(edge & (surface.seen(j) if need_seen else True))[0].tolist())
    return mask, x, y, surface.depth(j)


def camera_points(surface, i, near=None):
    """process_camera's Delaunay input (:401-423), in track order -> (track index [k], xy [k, 2])."""
    mask, x, y, _ = selected(surface, i, near=near)
    idx = np.nonzero(mask)[0]
    return idx, np.stack([x[idx], y[idx]], axis=1)


def depth_buffer(surface, j, near=None):
    """DepthBuffer::new (:262-318) -> [height, width] f64, NaN = None; the cell is the minimum of its depths."""
    mask, x, y, d = selected(surface, j, near=near)
    if not mask.any():
        return np.full((0, 0), np.nan)
    x, y, d = x[mask], y[mask], d[mask]
    w, h = int(as_usize(np.ceil(x.max()))) + 1, int(as_usize(np.ceil(y.max()))) + 1
    cx, cy = as_usize(rust_round(x)), as_usize(rust_round(y))
    flat = np.full(w * h, np.inf)
    np.minimum.at(flat, cy * w + cx, d)
    if near is not None:
        tr = np.nonzero(mask)[0]
        edge = ((x == x.max()) & _near_int(x)) | ((y == y.max()) & _near_int(y))  # the ceil that sizes the grid
        near.tracks.update(tr[_near_half(x) | _near_half(y) | edge].tolist())
        # two depths of one cell within TOL (and not the same number)
        order = np.lexsort((d, cy * w + cx))
        c_s, d_s = (cy * w + cx)[order], d[order]
        close = (c_s[1:] == c_s[:-1]) & (d_s[1:] != d_s[:-1]) & (d_s[1:] - d_s[:-1] <= TOL)
        near.cells.update((j, int(c) // w, int(c) % w) for c in c_s[1:][close])
    return np.where(np.isinf(flat), np.nan, flat).reshape(h, w)


# ---- ProjectedPolygon and its iterator (:107-254) ---------------------------------------------------------------------------------
def sort_vertices(pts):
    """ProjectedPolygon::new (:115-129): [k, 3, 3] (x, y, value) stably sorted by y with total_cmp."""
    order = np.argsort(total_key(pts[:, :, 1]), axis=1, kind="stable")
    return np.take_along_axis(pts, order[:, :, None], axis=1)


def walk(pts, max_x, max_y, near=None, chunk_rows=1 << 17, chunk_pixels=1 << 22):
    """The iterator over the polygons pts [k, 3, 3]: yields the emitted pixels as flat arrays (polygon [e], x [e], y [e],
    value [e]).  The rows of all polygons are flattened like the pixels of a row (in chunks that bound the memory): no
    Python loop runs over a polygon's rows or pixels."""
    if len(pts) == 0:
        return
    t = sort_vertices(np.asarray(pts, dtype=np.float64))
    ax, ay, av = t[:, 0, 0], t[:, 0, 1], t[:, 0, 2]
    bx, by, bv = t[:, 1, 0], t[:, 1, 1], t[:, 1, 2]
    cx, cy, cv = t[:, 2, 0], t[:, 2, 1], t[:, 2, 2]
    with np.errstate(all="ignore"):
        y0 = clamp_usize(np.floor(ay), max_y)               # :132
        y1 = clamp_usize(np.ceil(cy + 1.0), max_y)          # :133-135
        if near is not None:
            near.polygons.update(np.nonzero(_near_int(ay) | _near_int(by) | _near_int(cy))[0].tolist())  # floor / ceil, y at a.y, b.y, c.y
        nrows = np.maximum(y1 - y0, 0)
        total_rows = int(nrows.sum())
        poly_of = np.repeat(np.arange(len(t)), nrows)
        y_of = y0[poly_of] + (np.arange(total_rows) - np.repeat(np.cumsum(nrows) - nrows, nrows))
        for r0 in range(0, total_rows, chunk_rows):
            act, yi = poly_of[r0:r0 + chunk_rows], y_of[r0:r0 + chunk_rows]
            y = yi.astype(np.float64)
            on = ~((y < ay[act]) | (y > cy[act]))           # :186-188
            act, yi, y = act[on], yi[on], y[on]
            if len(act) == 0:
                continue
            a_x, a_y, a_v, b_x, b_y, b_v, c_x, c_y, c_v = (q[act] for q in (ax, ay, av, bx, by, bv, cx, cy, cv))
            first = (y < b_y) | (np.abs((b_y - c_y) / (b_x - c_x)) < EPS)  # :190
            k1 = (y - a_y) / (b_y - a_y)
            k2 = (y - b_y) / (c_y - b_y)
            sx = np.where(first, a_x * (1.0 - k1) + b_x * k1, b_x * (1.0 - k2) + c_x * k2)
            sv = np.where(first, a_v * (1.0 - k1) + b_v * k1, b_v * (1.0 - k2) + c_v * k2)
            k3 = (y - a_y) / (c_y - a_y)                    # :202-204
            ex = a_x * (1.0 - k3) + c_x * k3
            ev = a_v * (1.0 - k3) + c_v * k3
            keep = sx < ex                                  # :207-217
            start_x, end_x = np.where(keep, sx, ex), np.where(keep, ex, sx)
            start_v, end_v = np.where(keep, sv, ev), np.where(keep, ev, sv)
            x0 = clamp_usize(np.floor(start_x), max_x)      # :219-220
            x1 = clamp_usize(np.ceil(end_x + 1.0), max_x)
            cnt = np.maximum(x1 - x0, 0)
            if near is not None:
                near.polygons.update(act[(_near_int(start_x) | _near_int(end_x)) & (cnt > 0)].tolist())
            ends = np.cumsum(cnt)
            lo = 0
            while lo < len(act):                            # sub-chunks of at most ~chunk_pixels pixels (at least one row)
                hi = max(lo + 1, int(np.searchsorted(ends, (ends[lo - 1] if lo else 0) + chunk_pixels, side="right")))
                c = cnt[lo:hi]
                total = int(c.sum())
                if total:
                    rep = np.repeat(np.arange(lo, hi), c)
                    xs = x0[rep] + (np.arange(total) - np.repeat(np.cumsum(c) - c, c))
                    xc = (xs.astype(np.float64) - start_x[rep]) / (end_x[rep] - start_x[rep])  # :226
                    ok = (0.0 <= xc) & (xc <= 1.0)
                    value = start_v[rep] * (1.0 - xc) + xc * end_v[rep]
                    if near is not None:
                        close = np.isfinite(xc) & ((np.abs(xc) <= TOL) | (np.abs(xc - 1.0) <= TOL))
                        near.polygons.update(act[rep][close].tolist())
                    yield act[rep][ok], xs[ok], yi[rep][ok], value[ok]
                lo = hi


def polygon_points(surface, j, polygons, x, y, d):
    p = np.asarray(polygons, dtype=np.int64).reshape(-1, 3)
    return np.stack([x[p], y[p], d[p]], axis=2)  # [k, 3 vertices, (x, y, depth)]


def obstructs(surface, j, polygons, near=None, buffer=None):
    """polygon_obstructs (:320-353) of every polygon in camera j -> [k] bool."""
    buf = depth_buffer(surface, j, near=near) if buffer is None else buffer
    polygons = np.asarray(polygons, dtype=np.int64).reshape(-1, 3)
    out = np.zeros(len(polygons), dtype=bool)
    h, w = buf.shape
    if w * h == 0:
        return out
    x, y = surface.project(j)
    d = surface.depth(j)
    for p, xs, ys, value in walk(polygon_points(surface, j, polygons, x, y, d), w, h, near=near):
        cell = buf[ys, xs]
        with np.errstate(invalid="ignore"):
            margin = cell - value
            hit = margin > EPS  # (None: NaN, false)
        out[p[hit]] = True
        if near is not None:
            with np.errstate(invalid="ignore"):
                near.polygons.update(p[np.abs(margin - EPS) <= TOL].tolist())
    return out


def cull(surface, i, polygons, near=None):
    """The culling loop of process_camera (:457-508) -> (keep [k] bool, per camera (width, height, occupied, obstructing))."""
    polygons = np.asarray(polygons, dtype=np.int64).reshape(-1, 3)
    keep = np.ones(len(polygons), dtype=bool)
    stats = []
    for j in range(len(surface.cameras)):
        if j == i:
            stats.append((0, 0, 0, 0))
            continue
        buf = depth_buffer(surface, j, near=near)
        ob = obstructs(surface, j, polygons, near=near, buffer=buf)
        keep &= ~ob
        stats.append((buf.shape[1], buf.shape[0], int((~np.isnan(buf)).sum()), int(ob.sum())))
    return keep, stats


# ---- the polygon list (:50-105, 384, 510-516) ---------------------------------------------------------------------------------------
def rotate(v):
    """Polygon::new (:56-67)."""
    v = [int(q) for q in v]
    if v[0] < v[1] and v[0] < v[2]:
        return (v[0], v[1], v[2])
    if v[1] < v[0] and v[1] < v[2]:
        return (v[1], v[2], v[0])
    return (v[2], v[0], v[1])


def merge(per_camera):
    """per_camera: [(camera, polygons [k, 3])] in the order process_camera runs -> (polygons [p, 3], camera [p]): after each
    camera the list is sorted by vertices and de-duplicated by vertices (the lowest camera keeps a shared triple), at
    the end stably sorted by camera."""
    current = []  # (vertices, camera), sorted by vertices
    for cam, polys in per_camera:
        current = current + [(rotate(v), int(cam)) for v in np.asarray(polys).reshape(-1, 3)]
        current.sort(key=lambda pc: (pc[0], pc[1]))
        dedup = []
        for pc in current:
            if not dedup or dedup[-1][0] != pc[0]:
                dedup.append(pc)
        current = dedup
    current.sort(key=lambda pc: pc[1])  # stable
    polys = np.array([pc[0] for pc in current], dtype=np.uint32).reshape(-1, 3)
    return polys, np.array([pc[1] for pc in current], dtype=np.uint32)


def create(surface, triangulate, near=None):
    """Mesh::create (:363-387) with the caller's Delaunay -> (polygons, camera, per camera (track index, polygons, keep))."""
    kept, per = [], []
    for i in range(len(surface.cameras)):
        idx, xy = camera_points(surface, i, near=near)
        faces = np.asarray(triangulate(xy), dtype=np.int64).reshape(-1, 3)
        polys = idx[faces] if len(faces) else np.zeros((0, 3), dtype=np.int64)
        keep, _ = cull(surface, i, polys, near=near)
        kept.append((i, polys[keep]))
        per.append((idx, polys, keep))
    polygons, camera = merge(kept)
    return polygons, camera, per


# ---- ImageWriter (:1016-1143) --------------------------------------------------------------------------------------------------
def depth_image(surface, project_to_image, scale, polygons, near=None):
    """-> (map [height, width] f64 NaN = None, (min_x, min_y), min depth, max depth); None when no projection is in range
    ("No point projections found", :1046).  A cell is the maximum of what it receives."""
    mask, x, y, d = selected(surface, project_to_image, need_seen=False, near=near)
    if not mask.any():
        return None
    min_x, max_x, min_y, max_y = x[mask].min(), x[mask].max(), y[mask].min(), y[mask].max()
    w = int(as_usize(np.ceil(max_x) - np.floor(min_x))) + 1  # :1048-1049
    h = int(as_usize(np.ceil(max_y) - np.floor(min_y))) + 1
    px, py, pd = x - min_x, y - min_y, d * scale            # :1056-1058
    flat = np.full(w * h, -np.inf)
    dx = np.clip(as_usize(rust_round(px[mask])), 0, w - 1)   # :1059-1060
    dy = np.clip(as_usize(rust_round(py[mask])), 0, h - 1)
    np.maximum.at(flat, dy * w + dx, pd[mask])
    if near is not None:
        tr = np.nonzero(mask)[0]
        near.tracks.update(tr[_near_half(px[mask]) | _near_half(py[mask])].tolist())
        near.tracks.update(np.nonzero(mask & ((x == max_x) & _near_int(max_x) | (x == min_x) & _near_int(min_x)
                                              | (y == max_y) & _near_int(max_y) | (y == min_y) & _near_int(min_y)))[0].tolist())
    polygons = np.asarray(polygons, dtype=np.int64).reshape(-1, 3)
    drawn = mask[polygons].all(axis=1) if len(polygons) else np.zeros(0, dtype=bool)  # :1089-1096
    sel = np.nonzero(drawn)[0]
    pts = np.stack([px[polygons[sel]], py[polygons[sel]], pd[polygons[sel]]], axis=2) if len(sel) else np.zeros((0, 3, 3))
    sub = Near() if near is not None else None
    for p, xs, ys, value in walk(pts, w - 1, h - 1, near=sub):  # :1098-1102
        np.maximum.at(flat, ys * w + xs, value)
    if near is not None:
        near.polygons.update(int(sel[q]) for q in sub.polygons)
    out = np.where(np.isinf(flat), np.nan, flat).reshape(h, w)
    return out, (float(min_x), float(min_y)), float(np.nanmin(out)), float(np.nanmax(out))


# ---- near_threshold ----------------------------------------------------------------------------------------------------------
def near_threshold(surface, polygons, camera_i=None, project_to_image=None, scale=-1.0):
    """Near: the polygons, cells and tracks for which a deciding quantity lies within 1e-9 of its threshold - a floor, ceil
    or round argument next to an integer or a half, y at a.y / b.y / c.y, x_c at 0 or 1, cell - depth at EPSILON, two
    depths of one cell within 1e-9, a projection at the range edge - over the culling of camera_i's `polygons` (every
    other camera) and, with project_to_image, the depth image of `polygons`."""
    near = Near()
    if camera_i is not None:
        camera_points(surface, camera_i, near=near)
        cull(surface, camera_i, polygons, near=near)
    if project_to_image is not None:
        depth_image(surface, project_to_image, scale, polygons, near=near)
    return near
