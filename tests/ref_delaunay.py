"""The result of cvhip_mesh_delaunay, restated, in exact arithmetic on the CPU.

The faces of the Delaunay triangulation of the DISTINCT positions of xy ([k, 2] f64): counter-clockwise, the smallest index
first; of several indices at one position the lowest is the vertex; a maximal set of four or more points on one empty
circle is fanned from its lowest index.  Every sign is that of the exact determinant of the doubles: they are scaled to
Python ints by a common power of two, and a vectorised f64 evaluation with its forward error bound decides only what
lies above the bound.

check(xy, faces) -> violations; canonical(xy, faces) -> the faces with every tie polygon fanned as defined;
brute(xy) -> the definition by enumeration (k <= 40).  `check` empty and canonical == faces (as sets) say that `faces` is
THE defined result.
"""
from __future__ import annotations

import itertools

import numpy as np

EPS = 2.0 ** -53
ORIENT_BOUND = (3.0 + 16.0 * EPS) * EPS   # Shewchuk's stage-A bounds
CIRCLE_BOUND = (10.0 + 96.0 * EPS) * EPS
TINY = 1e-280


class Points:
    """xy with its exact integer image: X[i], Y[i] = xy[i] * 2^e for one e."""

    def __init__(self, xy):
        self.xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2) + 0.0  # (-0.0 -> 0.0)
        if not np.isfinite(self.xy).all():
            raise ValueError("non-finite coordinate")
        self.k = len(self.xy)
        self._hull = None
        ratios = [float(v).as_integer_ratio() for v in self.xy.ravel()]
        den = max([d for _, d in ratios], default=1)
        ints = [n * (den // d) for n, d in ratios]
        self.X, self.Y = ints[0::2], ints[1::2]
        # the vertex of every position: its lowest index
        if self.k:
            _, first, inverse = np.unique(self.xy, axis=0, return_index=True, return_inverse=True)
            lowest = np.full(len(first), self.k, dtype=np.int64)
            np.minimum.at(lowest, inverse.reshape(-1), np.arange(self.k))
            self.vertex = lowest[inverse.reshape(-1)]
        else:
            self.vertex = np.zeros(0, dtype=np.int64)
        self.distinct = np.flatnonzero(self.vertex == np.arange(self.k))

    # ---- exact, scalar ----
    def orient1(self, a, b, c):
        X, Y = self.X, self.Y
        d = (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a])
        return (d > 0) - (d < 0)

    def circle1(self, a, b, c, d):
        X, Y = self.X, self.Y
        ax, ay, bx, by, cx, cy = X[a] - X[d], Y[a] - Y[d], X[b] - X[d], Y[b] - Y[d], X[c] - X[d], Y[c] - Y[d]
        det = (ax * ax + ay * ay) * (bx * cy - cx * by) + (bx * bx + by * by) * (cx * ay - ax * cy) + (cx * cx + cy * cy) * (ax * by - bx * ay)
        return (det > 0) - (det < 0)

    def cross1(self, u, v):
        """x_u y_v - x_v y_u, an exact int (in units of 4^-e)"""
        return self.X[u] * self.Y[v] - self.X[v] * self.Y[u]

    # ---- exact, vectorised behind the f64 filter ----
    def orient(self, a, b, c):
        a, b, c = (np.asarray(v, dtype=np.int64) for v in (a, b, c))
        p = self.xy
        with np.errstate(all="ignore"):
            l = (p[b, 0] - p[a, 0]) * (p[c, 1] - p[a, 1])
            r = (p[b, 1] - p[a, 1]) * (p[c, 0] - p[a, 0])
            det = l - r
            sure = (np.abs(det) > ORIENT_BOUND * (np.abs(l) + np.abs(r))) & (np.abs(det) > TINY)
        out = np.sign(det).astype(np.int64)
        for i in np.flatnonzero(~sure):
            out[i] = self.orient1(int(a[i]), int(b[i]), int(c[i]))
        return out

    def circle(self, a, b, c, d):
        """+1 where d lies strictly inside the circle through a, b, c (counter-clockwise), 0 on it"""
        a, b, c, d = (np.asarray(v, dtype=np.int64) for v in (a, b, c, d))
        p = self.xy
        with np.errstate(all="ignore"):
            adx, ady = p[a, 0] - p[d, 0], p[a, 1] - p[d, 1]
            bdx, bdy = p[b, 0] - p[d, 0], p[b, 1] - p[d, 1]
            cdx, cdy = p[c, 0] - p[d, 0], p[c, 1] - p[d, 1]
            al, bl, cl = adx * adx + ady * ady, bdx * bdx + bdy * bdy, cdx * cdx + cdy * cdy
            det = al * (bdx * cdy - cdx * bdy) + bl * (cdx * ady - adx * cdy) + cl * (adx * bdy - bdx * ady)
            perm = (np.abs(bdx * cdy) + np.abs(cdx * bdy)) * al + (np.abs(cdx * ady) + np.abs(adx * cdy)) * bl + \
                   (np.abs(adx * bdy) + np.abs(bdx * ady)) * cl
            sure = (np.abs(det) > CIRCLE_BOUND * perm) & (np.abs(det) > TINY)
        out = np.sign(det).astype(np.int64)
        for i in np.flatnonzero(~sure):
            out[i] = self.circle1(int(a[i]), int(b[i]), int(c[i]), int(d[i]))
        return out

    def hull(self, subset=None):
        """The strict convex hull (monotone chain, exact), counter-clockwise, as indices; fewer than 3 for a degenerate set"""
        if subset is None and self._hull is not None:
            return self._hull
        idx = self.distinct if subset is None else np.asarray(sorted(set(int(v) for v in subset)), dtype=np.int64)
        if len(idx) < 3:
            return [int(v) for v in idx]
        idx = idx[np.lexsort((self.xy[idx, 1], self.xy[idx, 0]))]
        px, py = self.xy[:, 0].tolist(), self.xy[:, 1].tolist()  # (Python floats: the loop below is scalar)

        def turn(a, b, c):
            l = (px[b] - px[a]) * (py[c] - py[a])
            r = (py[b] - py[a]) * (px[c] - px[a])
            det = l - r
            if abs(det) > ORIENT_BOUND * (abs(l) + abs(r)) and abs(det) > TINY:
                return 1 if det > 0 else -1
            return self.orient1(a, b, c)

        def half(seq):
            out = []
            for v in seq:
                while len(out) >= 2 and turn(out[-2], out[-1], v) <= 0:
                    out.pop()
                out.append(v)
            return out

        order = [int(v) for v in idx]
        lower, upper = half(order), half(order[::-1])
        ring = lower[:-1] + upper[:-1]
        if subset is None:
            self._hull = ring
        return ring

    def hull_area2(self, ring=None):
        """twice the hull's area, an exact int"""
        ring = self.hull() if ring is None else ring
        if len(ring) < 3:
            return 0
        return sum(self.cross1(ring[i], ring[(i + 1) % len(ring)]) for i in range(len(ring)))


def rotate(faces):
    """Polygon::new's rotation: the smallest index first, the orientation kept"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if not len(f):
        return f
    s = np.argmin(f, axis=1)
    return np.stack([f[np.arange(len(f)), (s + i) % 3] for i in range(3)], axis=1)


def orient_faces(xy, faces):
    """Any triangles -> counter-clockwise and rotated (what scipy's simplices need before a comparison)"""
    P = xy if isinstance(xy, Points) else Points(xy)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3).copy()
    if len(f):
        cw = P.orient(f[:, 0], f[:, 1], f[:, 2]) < 0
        f[cw] = f[cw][:, [0, 2, 1]]
    return rotate(f)


def as_set(faces):
    return set(map(tuple, np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist()))


def _edges(f, k):
    """directed edges of the faces: keys u * k + v, the face and the apex of each"""
    u = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    v = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    apex = np.concatenate([f[:, 2], f[:, 0], f[:, 1]])
    face = np.tile(np.arange(len(f)), 3)
    return u, v, apex, face


def _pairs(f, k):
    """the interior edges: (u, v, apex of the face left of u->v, apex of the face right of it, the two faces), each once"""
    u, v, apex, face = _edges(f, k)
    key, rev = u * k + v, v * k + u
    order = np.argsort(key)
    pos = np.searchsorted(key[order], rev)
    pos[pos >= len(key)] = 0
    has = key[order][pos] == rev
    mate = order[pos]
    sel = has & (u < v)
    return u[sel], v[sel], apex[sel], apex[mate[sel]], face[sel], face[mate[sel]], (u[~has], v[~has])


def check(xy, faces, limit=5):
    """-> the list of violations (strings; at most `limit` of a kind) of `faces` against the definition, ties aside"""
    P = xy if isinstance(xy, Points) else Points(xy)
    k = P.k
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    bad = []

    def report(kind, rows):
        for r in list(rows)[:limit]:
            bad.append(f"{kind}: {r}")

    if len(f) and (f.min() < 0 or f.max() >= k):
        return ["a vertex out of range"]
    area2 = P.hull_area2()
    if not len(f):
        if area2 != 0:
            bad.append("no faces, but the points span an area")
        return bad
    report("not counter-clockwise", f[P.orient(f[:, 0], f[:, 1], f[:, 2]) <= 0].tolist())
    report("not rotated", f[(f[:, 0] > f[:, 1]) | (f[:, 0] > f[:, 2])].tolist())
    u, v, apex, face = _edges(f, k)
    key = u * k + v
    uniq, counts = np.unique(key, return_counts=True)
    report("directed edge used twice", [(int(q // k), int(q % k)) for q in uniq[counts > 1]])
    und = np.minimum(u, v) * k + np.maximum(u, v)
    uq, uc = np.unique(und, return_counts=True)
    report("edge in more than two faces", [(int(q // k), int(q % k)) for q in uq[uc > 2]])
    used = np.zeros(k, dtype=bool)
    used[f.ravel()] = True
    report("a duplicate's higher index is a vertex", np.flatnonzero(used & (P.vertex != np.arange(k))).tolist())
    report("a point in no face", np.flatnonzero(~used & (P.vertex == np.arange(k))).tolist())
    if bad:
        return bad
    eu, ev, w1, w2, _, _, (bu, bv) = _pairs(f, k)
    # the faces' doubled areas sum to the shoelace sum over the boundary edges: the interior edges cancel exactly
    if sum(P.cross1(int(a), int(b)) for a, b in zip(bu, bv)) != area2:
        bad.append("the faces' area is not the convex hull's")
    inside = P.circle(eu, ev, w1, w2) > 0
    report("not locally Delaunay", np.stack([eu, ev, w1, w2], axis=1)[inside].tolist())
    return bad


def _fan(P, members):
    """the co-circular points `members` as their convex polygon, fanned from its lowest index"""
    ring = P.hull(members)
    s = ring.index(min(ring))
    ring = ring[s:] + ring[:s]
    return [(ring[0], ring[i], ring[i + 1]) for i in range(1, len(ring) - 1)]


def canonical(xy, faces):
    """`faces` (which pass `check`) with every group of faces joined by an exact in-circle zero merged into its polygon and
    fanned from its lowest index -> [f, 3] int64"""
    P = xy if isinstance(xy, Points) else Points(xy)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if not len(f):
        return f
    eu, ev, w1, w2, f1, f2, _ = _pairs(f, P.k)
    tie = P.circle(eu, ev, w1, w2) == 0
    parent = list(range(len(f)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a, b in zip(f1[tie].tolist(), f2[tie].tolist()):
        parent[find(a)] = find(b)
    groups = {}
    for i in set(f1[tie].tolist()) | set(f2[tie].tolist()):
        groups.setdefault(find(i), []).append(i)
    keep = np.ones(len(f), dtype=bool)
    extra = []
    for members in groups.values():
        keep[members] = False
        extra += _fan(P, f[members].ravel().tolist())
    out = np.concatenate([f[keep], np.asarray(extra, dtype=np.int64).reshape(-1, 3)])
    return rotate(out)


def brute(xy):
    """The definition by enumeration (k <= 40): a triple of distinct positions is a face when no point lies strictly inside
    its circle; the points ON such a circle form a polygon, fanned from its lowest index -> [f, 3] int64, rotated"""
    P = xy if isinstance(xy, Points) else Points(xy)
    if P.k > 40:
        raise ValueError("brute is for 40 points or fewer")
    idx = P.distinct
    faces, polygons = set(), set()
    for a, b, c in itertools.combinations(idx.tolist(), 3):
        o = P.orient1(a, b, c)
        if o == 0:
            continue
        if o < 0:
            b, c = c, b
        n = len(idx)
        s = P.circle(np.full(n, a), np.full(n, b), np.full(n, c), idx)
        if (s > 0).any():
            continue
        on = idx[s == 0].tolist()  # (a, b, c themselves are on it)
        if len(on) == 3:
            faces.add((a, b, c))
        else:
            polygons.add(frozenset(on))
    for members in polygons:
        faces.update(_fan(P, members))
    return rotate(np.asarray(sorted(faces), dtype=np.int64).reshape(-1, 3))


# ---- the point sets the tests share --------------------------------------------------------------------------------------------
def circle50(seed=5):
    """the 12 integer points of x^2 + y^2 = 50 and three points outside, in a shuffled index order"""
    pts = [(sx * x, sy * y) for x, y in ((1, 7), (5, 5), (7, 1)) for sx in (1, -1) for sy in (1, -1)] + [(12, 3), (-11, -9), (2, 14)]
    rng = np.random.default_rng(seed)
    return np.asarray(pts, dtype=np.float64)[rng.permutation(len(pts))]


def circle50_ulp(seed=5):
    """circle50 with every coordinate nudged by one ulp, up or down"""
    xy = circle50(seed)
    rng = np.random.default_rng(seed + 1)
    return np.where(rng.random(xy.shape) < 0.5, np.nextafter(xy, np.inf), np.nextafter(xy, -np.inf))


def lattice(nx=17, ny=13):
    gx, gy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    return np.stack([gx.ravel(), gy.ravel()], axis=1)


def nearly_collinear(n=200, seed=9):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.0, 100.0, n), 1e-9 * rng.standard_normal(n)], axis=1)


def with_duplicates(seed=11):
    """60 random points, 20 of them repeated (some three times) at higher and lower indices -> (xy, number of duplicates)"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.0, 50.0, (60, 2))
    xy = np.concatenate([base, base[:20], base[10:15]])
    xy = xy[rng.permutation(len(xy))]
    return xy, 25


def unit_square_cases():
    """the unit square with the lowest index at each corner in turn, and the answers by hand: the fan from index 0, around
    the square counter-clockwise -> [(xy, faces)]"""
    A, B, C, D = (0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)  # counter-clockwise
    return [(np.array([A, B, C, D]), [(0, 1, 2), (0, 2, 3)]),
            (np.array([B, A, D, C]), [(0, 3, 2), (0, 2, 1)]),   # from B: C = 3, D = 2, A = 1
            (np.array([C, D, B, A]), [(0, 1, 3), (0, 3, 2)]),   # from C: D = 1, A = 3, B = 2
            (np.array([D, B, A, C]), [(0, 2, 1), (0, 1, 3)])]   # from D: A = 2, B = 1, C = 3
