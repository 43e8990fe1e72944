"""Restatement of PerspectiveTriangulation::merge_tracks (src/triangulation.rs:1421-1540) - test infrastructure, not
imported by cybervision_amd.

merge_tracks_literal transcribes the Rust fold for fold (AverageTrack::add_track / add_average_track / to_track,
:509-603, can_merge :347-368), for small grids.  merge_tracks is the numpy closed form of what those folds compute
(DESIGN.md 4.10): each fold returns the points of the LAST element it folded, so the area track of a cell is the highest
row of one cell and every kept cell yields a copy of its own highest row.

Tables: n x m x 2 int32, a point present iff x >= 0 and y >= 0.
"""
from __future__ import annotations

import numpy as np

MERGE_TRACKS_SEARCH_RADIUS = 2      # triangulation.rs:17
MERGE_TRACKS_MAX_DISTANCE = 10      # :18
TRACKS_RADIUS_DENOMINATOR = 1000    # :19


def radius_and_distance(width, height):
    """(search_radius, max_distance_sqr) of :1431-1443."""
    md = max(width, height)
    if md > TRACKS_RADIUS_DENOMINATOR:
        return (MERGE_TRACKS_SEARCH_RADIUS * md // TRACKS_RADIUS_DENOMINATOR,
                MERGE_TRACKS_MAX_DISTANCE * MERGE_TRACKS_MAX_DISTANCE * md // TRACKS_RADIUS_DENOMINATOR)
    return MERGE_TRACKS_SEARCH_RADIUS, MERGE_TRACKS_MAX_DISTANCE * MERGE_TRACKS_MAX_DISTANCE


# ---- literal transcription ----------------------------------------------------------------------------------------------
def _points(track):
    return [None if (x < 0 or y < 0) else (int(x), int(y)) for x, y in track]


class _AverageTrack:
    def __init__(self, images_count, points=None, count=0):
        self.points = points if points is not None else [None] * images_count
        self.count = count

    def add_track(self, src_track):  # :523-552
        points = [None] * len(self.points)
        for point_i in range(len(points)):
            dst_point = points[point_i]
            src_point = src_track[point_i]
            if src_point is None:
                continue
            if dst_point is not None:
                merged = ((dst_point[0][0] + src_point[0], dst_point[0][1] + src_point[1]), dst_point[1] + 1)
            else:
                merged = ((src_point[0], src_point[1]), 1)
            points[point_i] = merged
        return _AverageTrack(len(points), points, self.count + 1)

    def add_average_track(self, src_track):  # :554-583
        points = [None] * len(self.points)
        for point_i in range(len(points)):
            dst_point = points[point_i]
            src_point = src_track.points[point_i]
            if src_point is None:
                continue
            if dst_point is not None:
                merged = ((dst_point[0][0] + src_point[0][0], dst_point[0][1] + src_point[0][1]), src_point[1] + dst_point[1])
            else:
                merged = src_point
            points[point_i] = merged
        return _AverageTrack(len(points), points, self.count + src_track.count)

    def to_track(self):  # :585-602
        return [None if p is None else (p[0][0] // p[1], p[0][1] // p[1]) for p in self.points]


def _can_merge(a, b, max_distance_sqr):  # :347-368
    for p1, p2 in zip(a, b):
        if p1 is None or p2 is None:
            continue
        dx = max(p1[0], p2[0]) - min(p1[0], p2[0])
        dy = max(p1[1], p2[1]) - min(p1[1], p2[1])
        if dx * dx + dy * dy > max_distance_sqr:
            return False
    return True


def merge_tracks_literal(tracks, image_index, width, height):
    """merge_tracks as written -> the new table (k x m x 2 int32, (-1, -1) = None)."""
    tracks = np.asarray(tracks)
    m = tracks.shape[1]
    rows = [_points(t) for t in tracks]
    search_radius, max_distance_sqr = radius_and_distance(width, height)
    tracks_index = [[[] for _ in range(width)] for _ in range(height)]
    for track_i, track in enumerate(rows):  # :1444-1451
        point = track[image_index]
        if point is not None:
            if not (point[0] < width and point[1] < height):
                raise IndexError("Index out of bounds")
            tracks_index[point[1]][point[0]].append(track_i)
    vertical = [[None] * width for _ in range(height)]
    for point_y in range(height):  # :1458-1493
        for point_x in range(width):
            min_y = max(point_y - search_radius, 0)
            max_y = min(point_y + search_radius, height)
            acc = _AverageTrack(m)
            for y in range(min_y, max_y):
                inner = _AverageTrack(m)
                for point_track in tracks_index[y][point_x]:
                    inner = inner.add_track(rows[point_track])
                acc = acc.add_average_track(inner)
            vertical[point_y][point_x] = acc if acc.count > 0 else None
    out = []
    for point_y in range(height):  # :1496-1536, par_iter collected: row-major
        for point_x in range(width):
            point_tracks = tracks_index[point_y][point_x]
            if not point_tracks:
                continue
            min_x = max(point_x - search_radius, 0)
            max_x = min(point_x + search_radius, width)
            area = _AverageTrack(m)
            for x in range(min_x, max_x):
                if vertical[point_y][x] is not None:
                    area = area.add_average_track(vertical[point_y][x])
            if area.count == 0:
                continue
            area_track = area.to_track()
            can_merge = all(_can_merge(rows[t], area_track, max_distance_sqr) for t in point_tracks)
            avg = _AverageTrack(m)
            for t in point_tracks:
                avg = avg.add_track(rows[t])
            if can_merge:
                out.append(avg.to_track())
    table = np.full((len(out), m, 2), -1, dtype=np.int32)
    for k, track in enumerate(out):
        for j, p in enumerate(track):
            if p is not None:
                table[k, j] = p
    return table


# ---- closed form ----------------------------------------------------------------------------------------------------------
def merge_tracks(tracks, image_index, width, height):
    """The six steps of DESIGN.md 4.10, vectorised -> (out_rows int64, stats (present, cells, rejected, empty_area)).
    The new table is tracks[out_rows]."""
    tracks = np.asarray(tracks)
    n = len(tracks)
    w, h = int(width), int(height)
    r, d2 = radius_and_distance(w, h)
    pi = tracks[:, image_index] if n else np.zeros((0, 2), dtype=np.int32)
    present = (pi[:, 0] >= 0) & (pi[:, 1] >= 0)
    prow = np.flatnonzero(present)
    px, py = pi[prow, 0].astype(np.int64), pi[prow, 1].astype(np.int64)
    if ((px >= w) | (py >= h)).any():
        raise IndexError("Index out of bounds")
    cell = py * w + px
    # 1. last(p): the highest row of each cell, +1 (0 = empty)
    last = np.zeros(w * h, dtype=np.int64)
    if len(cell):
        ucell, first_rev = np.unique(cell[::-1], return_index=True)
        last[ucell] = prow[::-1][first_rev] + 1
    last2 = last.reshape(h, w)
    # 2-3. column occupancy over rows [y - r, min(y + r, h)), then x* = the highest occupied column <= min(px + r, w) - 1
    cs = np.zeros((h + 1, w), dtype=np.int32)
    np.cumsum(last2 > 0, axis=0, out=cs[1:])
    ys = np.arange(h)
    colocc = (cs[np.minimum(ys + r, h)] - cs[np.maximum(ys - r, 0)]) > 0
    prev = np.where(colocc, np.arange(w, dtype=np.int32)[None, :], -1)
    np.maximum.accumulate(prev, axis=1, out=prev)
    occ_cells = np.flatnonzero(last)
    ox, oy = occ_cells % w, occ_cells // w
    xhi = np.minimum(ox + r, w)
    yhi = np.minimum(oy + r, h)
    xs = prev[oy, xhi - 1]
    # 4. the area track A = last(x*, yhi - 1)
    area = np.zeros(w * h, dtype=np.int64)
    area[occ_cells] = last2[yhi - 1, xs]
    # 5. can_merge of every track of the cell with A
    keep = last > 0
    a = area[cell]
    chk = a > 0
    if chk.any():
        t1 = tracks[prow[chk]].astype(np.int64)
        t2 = tracks[a[chk] - 1].astype(np.int64)
        both = (t1[..., 0] >= 0) & (t1[..., 1] >= 0) & (t2[..., 0] >= 0) & (t2[..., 1] >= 0)
        dist = ((t1 - t2) ** 2).sum(axis=2)
        fail = (both & (dist > d2)).any(axis=1)
        keep[cell[chk][fail]] = False
    # 6. kept cells in row-major order, each a copy of its highest row
    kept = np.flatnonzero(keep)
    out_rows = last[kept] - 1
    stats = (int(len(prow)), int(len(occ_cells)), int(len(occ_cells) - len(kept)), int((area[occ_cells] == 0).sum()))
    return out_rows, stats
