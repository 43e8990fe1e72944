"""Restatement of what Mesh::output writes through an ObjWriter (src/output.rs:521-559, 774-1007): the Wavefront OBJ file image
and the .mtl text, each twice - `obj_bytes` with numpy arithmetic and formatter (a), `obj_bytes_scalar` as a transcription of
the writer's loops with one Python float operation per written operation and formatter (b).  The device's output
(cvhip_mesh_obj, cvhip_mesh_obj_mtl, cvhip_f64_display) must equal these byte for byte.

`{}` of an f64 in Rust is the shortest decimal digit string that reads back as the same double, the closest such one, laid out
without an exponent.  Python's repr(float) finds the same digits with code of its own (David Gay's); only the layout differs:
 (a) `display_a`: digits and exponent taken out of repr's text, laid out by hand;
 (b) `display_b`: format(Decimal(repr(x)), 'f') with the trailing ".0" or trailing zeros stripped.

images_or_dims: per image of a track a [height, width, 3] uint8 array or a (width, height) pair (pairs do for every mode but
Color).  A present point of a track is one with x >= 0."""
from __future__ import annotations

import math
from decimal import Decimal

import numpy as np

PLAIN, COLOR, TEXTURE = 0, 1, 2


class TrackHasNoImages(Exception):
    """the reference's error "Track has no images" (:908, :961)"""


# ---- `{}` of an f64 ------------------------------------------------------------------------------------------------------------------

def _special(x):
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    if x == 0.0:
        return "-0" if math.copysign(1.0, x) < 0 else "0"
    return None


def digits_exponent(x):
    """-> (digits without trailing zeros, exponent of the last digit) of repr(|x|), x finite and not zero"""
    text = repr(abs(x))
    mantissa, _, exp = text.partition("e")
    whole, _, frac = mantissa.partition(".")
    digits = (whole + frac).lstrip("0")
    e10 = (int(exp) if exp else 0) - len(frac)
    stripped = digits.rstrip("0")
    return stripped, e10 + len(digits) - len(stripped)


def display_a(x):
    x = float(x)
    special = _special(x)
    if special is not None:
        return special
    digits, e10 = digits_exponent(x)
    sign = "-" if x < 0 else ""
    point = len(digits) + e10
    if e10 >= 0:
        return sign + digits + "0" * e10
    if point > 0:
        return sign + digits[:point] + "." + digits[point:]
    return sign + "0." + "0" * -point + digits


def display_b(x):
    x = float(x)
    special = _special(x)
    if special is not None:
        return special
    text = format(Decimal(repr(x)), "f")
    if "." in text:
        text = text.rstrip("0").rstrip(".")
    return text


# ---- the .mtl text (:856-868) --------------------------------------------------------------------------------------------------------

def mtl_bytes(stem, m):
    out = []
    for i in range(m):
        name = f"{stem}-{i}.png"
        out += [f"newmtl Textured{i}", "Ka 0.2 0.2 0.2", "Kd 0.8 0.8 0.8", "Ks 1.0 1.0 1.0", "illum 2", "Ns 0.000500", f"map_Ka {name}",
                f"map_Kd {name}", ""]
    return "".join(line + "\n" for line in out).encode("utf-8")


def mtl_bytes_scalar(stem, m):
    text = ""
    for img_i in range(m):
        image_filename = stem + "-" + str(img_i) + ".png"
        text += "newmtl Textured" + str(img_i) + "\n"
        text += "Ka 0.2 0.2 0.2\n" + "Kd 0.8 0.8 0.8\n" + "Ks 1.0 1.0 1.0\n" + "illum 2\n" + "Ns 0.000500\n"
        text += "map_Ka " + image_filename + "\n"
        text += "map_Kd " + image_filename + "\n"
        text += "\n"
    return text.encode("utf-8")


# ---- the file image ------------------------------------------------------------------------------------------------------------------

def dims_of(images_or_dims):
    """-> [(width, height)] of arrays or pairs"""
    return [(int(im.shape[1]), int(im.shape[0])) if hasattr(im, "shape") else (int(im[0]), int(im[1])) for im in images_or_dims]


def _arrays(points, tracks, polygons, camera):
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    tracks = np.asarray(tracks, dtype=np.int64) if tracks is not None else np.zeros((len(points), 0, 2), np.int64)
    if tracks.ndim != 3:
        tracks = tracks.reshape(len(points), -1, 2) if len(points) else np.zeros((0, 0, 2), np.int64)
    polygons = np.asarray(polygons, dtype=np.int64).reshape(-1, 3)
    camera = np.asarray(camera if camera is not None else np.zeros(len(polygons)), dtype=np.int64).reshape(-1)
    return points, tracks, polygons, camera


def obj_sections(data, mode):
    """-> [header, v, vt, f] byte counts of a file image, by its lines' first words"""
    sizes = [0, 0, 0, 0]
    for line in data.split(b"\n")[:-1]:
        word = line.split(b" ", 1)[0]
        sizes[{b"mtllib": 0, b"v": 1, b"vt": 2, b"usemtl": 3, b"f": 3}[word]] += len(line) + 1
    return sizes


def obj_bytes(points, tracks, images_or_dims, mode, out_scale, polygons, camera, stem):
    """The file image with numpy arithmetic and display_a."""
    points, tracks, polygons, camera = _arrays(points, tracks, polygons, camera)
    n, m = tracks.shape[:2]
    show = display_a
    lines = []
    if mode == TEXTURE:
        lines.append(f"mtllib {stem}.mtl")
    xyz = np.stack([points[:, 0] * out_scale[0], (-points[:, 1]) * out_scale[1], points[:, 2] * out_scale[2]], axis=1)
    present = tracks[:, :, 0] >= 0
    if mode != PLAIN and n and not present.any(axis=1).all():
        raise TrackHasNoImages("Track has no images")
    colour = [None] * n
    if mode == COLOR and n:
        first = present.argmax(axis=1)
        xy = tracks[np.arange(n), first]
        x, y = xy[:, 0] & 0xFFFFFFFF, xy[:, 1] & 0xFFFFFFFF
        for c, image in enumerate(images_or_dims):
            h, w = image.shape[:2]
            for i in np.flatnonzero((first == c) & (x < w) & (y < h)):
                colour[i] = image[y[i], x[i]].astype(np.float64) / 255.0
    for i in range(n):
        text = "v " + " ".join(show(v) for v in xyz[i])
        if colour[i] is not None:
            text += " " + " ".join(show(v) for v in colour[i])
        lines.append(text)
    uv_index = np.zeros(n + 1, dtype=np.int64)
    if mode == TEXTURE:
        dims = np.array(dims_of(images_or_dims), dtype=np.int64).reshape(-1, 2)
        with np.errstate(all="ignore"):
            u = (tracks[:, :, 0] & 0xFFFFFFFF).astype(np.float64) / dims[None, :, 0].astype(np.float64)
            v = 1.0 - (tracks[:, :, 1] & 0xFFFFFFFF).astype(np.float64) / dims[None, :, 1].astype(np.float64)
        for i, c in zip(*np.nonzero(present)):
            lines.append(f"vt {show(u[i, c])} {show(v[i, c])}")
        uv_index[1:] = np.cumsum(present.sum(axis=1))
    before = np.concatenate([np.zeros((n, 1), dtype=np.int64), np.cumsum(present, axis=1)], axis=1)  # [n, m + 1]: present points below c
    current = None
    for p, cam in zip(polygons, camera):
        if mode == TEXTURE and cam != current:
            lines.append(f"usemtl Textured{cam}")
            current = cam
        text = "f"
        for k in (2, 1, 0):
            text += f" {p[k] + 1}"
            if mode == TEXTURE:
                text += f"/{uv_index[p[k]] + before[p[k], min(cam, m)] + 1}"
        lines.append(text)
    return "".join(line + "\n" for line in lines).encode("utf-8")


def _div(a, b):
    """IEEE a / b for Python floats (0 / 0 = NaN, x / 0 = inf)"""
    if b == 0.0:
        return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def obj_bytes_scalar(points, tracks, images_or_dims, mode, out_scale, polygons, camera, stem):
    """ObjWriter call by call (:877-997) with display_b."""
    points, tracks, polygons, camera = _arrays(points, tracks, polygons, camera)
    show = display_b
    out = ""
    if mode == TEXTURE:                                                       # output_header
        out += "mtllib " + stem + ".mtl\n"
    for i, p in enumerate(points):                                            # output_vertex
        color = None
        if mode == COLOR:
            found = next(((c, q) for c, q in enumerate(tracks[i]) if q[0] >= 0), None)
            if found is None:
                raise TrackHasNoImages("Track has no images")
            c, q = found
            x, y = int(q[0]) & 0xFFFFFFFF, int(q[1]) & 0xFFFFFFFF
            h, w = images_or_dims[c].shape[:2]
            if x < w and y < h:                                               # get_pixel_checked
                color = [int(v) for v in images_or_dims[c][y, x]]
        x, y, z = float(p[0]) * float(out_scale[0]), (-float(p[1])) * float(out_scale[1]), float(p[2]) * float(out_scale[2])
        out += "v " + show(x) + " " + show(y) + " " + show(z)
        if color is not None:
            out += " " + show(float(color[0]) / 255.0) + " " + show(float(color[1]) / 255.0) + " " + show(float(color[2]) / 255.0)
        out += "\n"
    uv_index = [0]
    if mode == TEXTURE:                                                       # output_vertex_uv
        dims = dims_of(images_or_dims)
        for i in range(len(points)):
            projections_count = 0
            for image_i, q in enumerate(tracks[i]):
                if q[0] < 0:
                    continue
                w, h = dims[image_i]
                projections_count += 1
                u = _div(float(int(q[0]) & 0xFFFFFFFF), float(w))
                v = 1.0 - _div(float(int(q[1]) & 0xFFFFFFFF), float(h))
                out += "vt " + show(u) + " " + show(v) + "\n"
            if projections_count == 0:
                raise TrackHasNoImages("Track has no images")
            uv_index.append(uv_index[-1] + projections_count)
    current_image = None
    for vertices, camera_i in zip(polygons, camera):                          # output_face
        camera_i = int(camera_i)
        if camera_i != current_image:
            if mode == TEXTURE:                                               # switch_material
                out += "usemtl Textured" + str(camera_i) + "\n"
            current_image = camera_i
        out += "f"
        for k in (2, 1, 0):
            index = int(vertices[k]) + 1
            if mode == TEXTURE:
                track = tracks[int(vertices[k])]
                uv = uv_index[int(vertices[k])] + sum(1 for q in track[:camera_i] if q[0] >= 0) + 1   # get_uv_index
                out += " " + str(index) + "/" + str(uv)
            else:
                out += " " + str(index)
        out += "\n"
    return out.encode("utf-8")
