"""Numpy restatement of what output::output writes (src/output.rs): PlyWriter's binary file image (:648-772, Mesh::output
:521-559) and ImageWriter::complete's colour mapping (:1117-1229), each twice - vectorised, and as a slow scalar
transcription with struct.pack('>d') and one Python float operation per written operation.  Every operation is a single
IEEE f64 operation or a byte move, so the device's output (cvhip_mesh_ply, cvhip_mesh_colour_map) must
equal these byte for byte.

images: a list of [height, width, 3] uint8 arrays, one per image of a track (None outside Color mode).  A None cell of a
depth map is NaN.  The colour table is an argument ([256, 3] uint8); `generated_table` is the generated, non-monotone one the
tests use (no table is shipped)."""
from __future__ import annotations

import math
import struct

import numpy as np

PLAIN, COLOR, TEXTURE = 0, 1, 2


class TrackHasNoImages(Exception):
    """the reference's error "Track has no images" (:726)"""


def generated_table():
    i = np.arange(256)
    return np.stack([(37 * i + 11) % 256, (101 * i + 7) % 256, (201 * i) % 256], axis=1).astype(np.uint8)


def header(n, n_poly, mode):
    """PlyWriter::output_header (:687-710)"""
    lines = ["ply", "format binary_big_endian 1.0", "comment Cybervision 3D surface", f"element vertex {n}",
             "property double x", "property double y", "property double z"]
    if mode == COLOR:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    lines += [f"element face {n_poly}", "property list uchar int vertex_indices", "end_header"]
    return "".join(line + "\n" for line in lines).encode("ascii")


def header_length(n, n_poly, mode):
    return 198 + len(str(n)) + len(str(n_poly)) + (60 if mode == COLOR else 0)


def first_points(tracks):
    """-> (first [n]: the lowest image index with tracks[i][c].x >= 0, -1 without one; xy [n, 2] there)."""
    tracks = np.asarray(tracks).reshape(len(tracks), -1, 2)
    n, m = tracks.shape[:2]
    if m == 0:
        return np.full(n, -1, dtype=np.int64), np.zeros((n, 2), dtype=np.int64)
    present = tracks[:, :, 0] >= 0
    first = np.where(present.any(axis=1), present.argmax(axis=1), -1)
    xy = tracks[np.arange(n), np.maximum(first, 0)].astype(np.int64)
    return first, xy


def vertex_colours(tracks, images):
    """-> (has [n] bool: get_pixel_checked succeeded, rgb [n, 3] uint8).  Raises TrackHasNoImages (:716-727)."""
    first, xy = first_points(tracks)
    if (first < 0).any():
        raise TrackHasNoImages("Track has no images")
    n = len(first)
    has, rgb = np.zeros(n, dtype=bool), np.zeros((n, 3), dtype=np.uint8)
    for c, image in enumerate(images):
        h, w = image.shape[:2]
        x, y = xy[:, 0].astype(np.uint32).astype(np.int64), xy[:, 1].astype(np.uint32).astype(np.int64)  # (Point2D<u32>)
        sel = (first == c) & (x < w) & (y < h)
        has[sel] = True
        rgb[sel] = image[y[sel], x[sel]]
    return has, rgb


def ply_bytes(points, tracks, images, mode, out_scale, polygons):
    """The file image: header, one record per track in track order, one per polygon in list order (vectorised)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    polygons = np.asarray(polygons, dtype=np.uint32).reshape(-1, 3)
    n = len(points)
    xyz = np.stack([points[:, 0] * out_scale[0], (-points[:, 1]) * out_scale[1], points[:, 2] * out_scale[2]], axis=1)
    if mode == COLOR and n:
        has, rgb = vertex_colours(tracks, images)
        rec = np.zeros(n, dtype=[("xyz", ">f8", 3), ("rgb", "u1", 3)])
        rec["xyz"], rec["rgb"] = xyz, rgb
        keep = np.ones((n, 27), dtype=bool)
        keep[~has, 24:] = False
        vertices = rec.view(np.uint8).reshape(n, 27)[keep].tobytes()
    else:
        vertices = xyz.astype(">f8").tobytes()
    face = np.zeros(len(polygons), dtype=[("count", "u1"), ("v", ">u4", 3)])
    face["count"], face["v"] = 3, polygons[:, ::-1]
    return header(n, len(polygons), mode) + vertices + face.tobytes()


def ply_bytes_scalar(points, tracks, images, mode, out_scale, polygons):
    """PlyWriter line by line (:687-763)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    polygons = np.asarray(polygons, dtype=np.uint32).reshape(-1, 3)
    tracks = np.asarray(tracks).reshape(len(points), -1, 2) if tracks is not None else None
    out = bytearray(header(len(points), len(polygons), mode))
    for i, p in enumerate(points):
        color = None
        if mode == COLOR:
            found = next(((c, q) for c, q in enumerate(tracks[i]) if q[0] >= 0), None)
            if found is None:
                raise TrackHasNoImages("Track has no images")
            c, q = found
            x, y = int(q[0]) & 0xFFFFFFFF, int(q[1]) & 0xFFFFFFFF
            h, w = images[c].shape[:2]
            if x < w and y < h:                                  # get_pixel_checked
                color = bytes(int(v) for v in images[c][y, x])
        x, y, z = float(p[0]) * float(out_scale[0]), (-float(p[1])) * float(out_scale[1]), float(p[2]) * float(out_scale[2])
        out += struct.pack(">d", x) + struct.pack(">d", y) + struct.pack(">d", z)
        if color is not None:
            out += color
    for v in polygons:
        out += b"\x03" + struct.pack(">I", int(v[2])) + struct.pack(">I", int(v[1])) + struct.pack(">I", int(v[0]))
    return bytes(out)


def parse_header(data):
    """-> (header bytes, n, n_poly, coloured) of a file image."""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    n = int(next(line for line in lines if line.startswith("element vertex ")).split()[2])
    n_poly = int(next(line for line in lines if line.startswith("element face ")).split()[2])
    return end, n, n_poly, "property uchar red" in lines


# ---- the colour map --------------------------------------------------------------------------------------------------------------

def _div(a, b):
    """IEEE a / b for Python floats (0 / 0 = NaN, x / 0 = +-inf)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _round_half_away(v):
    """f64::round: v - trunc(v) is exact, so the comparison with 0.5 is too"""
    if not math.isfinite(v):
        return v
    t = float(math.trunc(v))
    return t + math.copysign(1.0, v) if abs(v - t) >= 0.5 else t


def map_color_scalar(column, value):
    """map_color (:1218-1229) on one channel's 256 entries"""
    if value >= 1.0:
        return int(column[255])
    step = 1.0 / 255.0
    q = _div(value, step)
    q = math.floor(q) if math.isfinite(q) else q
    box = 0 if (q != q or q < 0.0) else (254 if q >= 254.0 else int(q))      # `as usize` saturates, NaN -> 0; clamp(0, 254)
    ratio = _div(value - step * float(box), step)
    c1, c2 = float(column[box]), float(column[box + 1])
    r = _round_half_away(c2 * ratio + c1 * (1.0 - ratio))
    return 0 if (r != r or r < 0.0) else (255 if r >= 255.0 else int(r))     # `as u8` saturates, NaN -> 0


def colour_map_scalar(depth_map, min_depth, max_depth, table):
    """ImageWriter::complete's loop (:1130-1140) cell by cell -> [h, w, 4] uint8"""
    depth_map = np.asarray(depth_map, dtype=np.float64)
    out = np.zeros(depth_map.shape + (4,), dtype=np.uint8)
    for idx in np.ndindex(depth_map.shape):
        depth = float(depth_map[idx])
        if depth != depth:
            continue
        value = _div(depth - float(min_depth), float(max_depth) - float(min_depth))
        out[idx] = [map_color_scalar(table[:, k], value) for k in range(3)] + [255]
    return out


def colour_map(depth_map, min_depth, max_depth, table):
    """The same, vectorised."""
    depth_map = np.asarray(depth_map, dtype=np.float64)
    table = np.asarray(table, dtype=np.uint8).reshape(256, 3)
    some = ~np.isnan(depth_map)
    out = np.zeros(depth_map.shape + (4,), dtype=np.uint8)
    with np.errstate(all="ignore"):
        value = (depth_map - np.float64(min_depth)) / (np.float64(max_depth) - np.float64(min_depth))
        step = np.float64(1.0) / np.float64(255.0)
        q = np.floor(value / step)
        box = np.where(q > 0.0, np.minimum(q, 254.0), 0.0)
        box = np.where(np.isnan(box), 0.0, box).astype(np.int64)
        ratio = (value - step * box.astype(np.float64)) / step
        for k in range(3):
            c1, c2 = table[box, k].astype(np.float64), table[box + 1, k].astype(np.float64)
            v = c2 * ratio + c1 * (1.0 - ratio)
            t = np.trunc(v)                                                 # half away from zero: v - trunc(v) is exact
            r = np.where(np.abs(v - t) >= 0.5, t + np.copysign(1.0, v), t)
            r = np.where(np.isnan(r), 0.0, np.clip(r, 0.0, 255.0)).astype(np.uint8)
            out[..., k] = np.where(value >= 1.0, table[255, k], r)
    out[..., 3] = 255
    out[~some] = 0
    return out
