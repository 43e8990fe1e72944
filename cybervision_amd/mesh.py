"""The mesh stage of output::output (src/output.rs:567-611) over the C ABI: the Delaunay input of a
camera, the occlusion culling of its polygons against the other cameras' depth buffers, the polygon list of Mesh::create
and ImageWriter's depth map.  The Delaunay construction is a callback (`triangulate`): `delaunay_scipy` (the default of
reconstruct_perspective_mesh) is one, `delaunay_device(device)` - cvhip_mesh_delaunay, DESIGN.md 4.13 - runs on the device
and needs no scipy.
The mesh output: `ply` / `write_ply` - PlyWriter's binary file image - and `colour_map` /
`depth_image_rgba` - ImageWriter::complete's colours; the colour table is the caller's.  `obj` / `write_obj` / `obj_mtl` - ObjWriter's
Wavefront OBJ text and its .mtl, `f64_display` - the decimal text of doubles that it rests on.  `png` / `write_png` /
`write_depth_png` - the PNG file image of the textures and of the depth map.  `jpeg` / `write_jpeg` /
`write_depth_jpeg` - the baseline JPEG file image, libjpeg's file, of the depth map.  `tiff` / `write_tiff` /
`write_depth_tiff` - the TIFF file image, uncompressed, LZW or PackBits, of the depth map.
No compute in Python - array bookkeeping and the calls only.

Defined where the reference's result depends on its thread order: a depth-buffer cell is the minimum of its depths (a
depth-image cell the maximum), and a triple that two cameras produce stays with the lowest camera.
"""
from __future__ import annotations

import ctypes as C
import enum

import numpy as np

from . import _lib

GRID_LANES = 262144                # CVHIP_MESH_GRID_LANES: lanes of one grid-stride launch
WIDE_THRESHOLD_DEFAULT = 2048      # CVHIP_MESH_WIDE_THRESHOLD_DEFAULT
WIDE_ALL, WIDE_NONE = 0, 0xFFFFFFFF
STATS = ("width", "height", "occupied", "dropped", "wide")
DELAUNAY_LANE_CELLS_DEFAULT = 1024  # CVHIP_MESH_DELAUNAY_LANE_CELLS_DEFAULT
LANE_CELLS_HOST, LANE_CELLS_UNBOUNDED = 0, 0xFFFFFFFF
DELAUNAY_LATTICE_DEFAULT = False    # CVHIP_MESH_DELAUNAY_LATTICE_DEFAULT
DELAUNAY_STATS = ("grid_width", "grid_height", "device_stars", "host_stars", "duplicates", "most_cells")  # CVHIP_DELAUNAY_STAT_*


class VertexMode(enum.IntEnum):
    """VertexMode (output.rs) as cvhip_mesh_ply and cvhip_mesh_obj take it (CVHIP_VERTEX_*).  In a PLY, Texture writes what Plain
    writes; in an OBJ it adds the vt table, the usemtl groups and the .mtl file."""
    Plain = 0
    Color = 1
    Texture = 2


def _p(a):
    if hasattr(a, "data_ptr"):  # a device tensor (_surface_array)
        return C.c_void_p(a.data_ptr()) if a.numel() else None
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _surface_array(a, dtype):
    """A surface's points or tracks as the entries take them: a contiguous device tensor as it is - its address goes to the
    library, which takes device pointers there -, anything else as a contiguous numpy array of `dtype`."""
    if hasattr(a, "data_ptr") and a.is_cuda and a.is_contiguous():
        return a
    if hasattr(a, "data_ptr"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def _surface_args(surface, image_shapes):
    """(points, tracks, n, m, projection, r, t, image_dims) as every cvhip_mesh_* entry takes them, and the arrays kept
    alive."""
    pts = _surface_array(surface.points, np.float64).reshape(-1, 3)
    tracks = _surface_array(surface.tracks, np.int32)
    m = len(surface.cameras)
    P = np.ascontiguousarray(np.stack([np.asarray(c.projection, dtype=np.float64).reshape(12) for c in surface.cameras])) \
        if m else np.zeros((0, 12))
    r = np.ascontiguousarray(np.stack([np.asarray(c.r, dtype=np.float64).reshape(3) for c in surface.cameras])) if m else np.zeros((0, 3))
    t = np.ascontiguousarray(np.stack([np.asarray(c.t, dtype=np.float64).reshape(3) for c in surface.cameras])) if m else np.zeros((0, 3))
    dims = np.ascontiguousarray(np.asarray(image_shapes, dtype=np.uint32).reshape(-1, 2))
    if len(dims) != m:
        raise ValueError("one (width, height) per camera")
    keep = (pts, tracks, P, r, t, dims)
    one = np.zeros(1)  # (the arrays of m = 0 still need an address: the library reports the error)
    args = [_p(pts), _p(tracks), len(pts), m] + [C.c_void_p((a if a.size else one).ctypes.data) for a in (P, r, t)] + \
           [C.c_void_p((dims if dims.size else one.view(np.uint32)).ctypes.data)]
    return args, keep


def set_wide_threshold(device, pixels: int):
    """cvhip_mesh_set_wide_threshold: polygons whose bounding box in the buffer holds `pixels` or more take the wave path
    (WIDE_ALL = 0: all, WIDE_NONE: none)."""
    _lib.check(_lib.lib().cvhip_mesh_set_wide_threshold(device.handle, int(pixels)), "cvhip_mesh_set_wide_threshold")


def camera_points(device, surface, image_shapes, camera_i: int):
    """The Delaunay input of camera_i (process_camera, :401-423) in track order -> (track index [k] uint32, xy [k, 2])."""
    args, _keep = _surface_args(surface, image_shapes)
    n = C.c_uint64(0)
    L = _lib.lib()
    _lib.check(L.cvhip_mesh_camera_points(device.handle, *args, int(camera_i), None, None, 0, C.byref(n)), "cvhip_mesh_camera_points")
    k = n.value
    index, xy = np.zeros(k, dtype=np.uint32), np.zeros((k, 2))
    if k:
        _lib.check(L.cvhip_mesh_camera_points(device.handle, *args, int(camera_i), _p(index), _p(xy), k, C.byref(n)),
                   "cvhip_mesh_camera_points")
    return index, xy


def depth_buffer(device, surface, image_shapes, camera_j: int):
    """DepthBuffer::new (:262-318) of camera_j -> [height, width] f64, NaN = None ((0, 0) without points)."""
    args, _keep = _surface_args(surface, image_shapes)
    w, h = C.c_uint64(0), C.c_uint64(0)
    L = _lib.lib()
    _lib.check(L.cvhip_mesh_depth_buffer(device.handle, *args, int(camera_j), None, 0, C.byref(w), C.byref(h)), "cvhip_mesh_depth_buffer")
    buf = np.zeros((h.value, w.value))
    if buf.size:
        _lib.check(L.cvhip_mesh_depth_buffer(device.handle, *args, int(camera_j), _p(buf), buf.size, C.byref(w), C.byref(h)),
                   "cvhip_mesh_depth_buffer")
    return buf


def cull(device, surface, image_shapes, camera_i: int, polygons):
    """The culling of camera_i's polygons ([k, 3] track indices) against every other camera (:457-508)
    -> (keep [k] bool, stats: per camera a dict of STATS; camera_i's is all zero)."""
    args, _keep = _surface_args(surface, image_shapes)
    poly = np.ascontiguousarray(polygons, dtype=np.uint32).reshape(-1, 3)
    keep = np.zeros(len(poly), dtype=np.uint8)
    m = args[3]
    stats = np.zeros((max(m, 1), 5), dtype=np.uint64)
    _lib.check(_lib.lib().cvhip_mesh_cull(device.handle, *args, int(camera_i), _p(poly), len(poly), _p(keep), _p(stats)),
               "cvhip_mesh_cull")
    return keep.astype(bool), [dict(zip(STATS, (int(v) for v in stats[j]))) for j in range(m)]


def merge(device, polygons, camera):
    """Mesh::create's list (:50-105, 384, 510-516) from the kept polygons of every camera ([k, 3]) and their cameras ([k])
    -> (polygons [k', 3] uint32, camera [k'] uint32): rotated, de-duplicated (the lowest camera wins), grouped by camera."""
    poly = np.ascontiguousarray(polygons, dtype=np.uint32).reshape(-1, 3)
    cam = np.ascontiguousarray(camera, dtype=np.uint32).reshape(-1)
    if len(cam) != len(poly):
        raise ValueError("one camera per polygon")
    out_p, out_c = np.zeros_like(poly), np.zeros_like(cam)
    n = C.c_uint64(0)
    _lib.check(_lib.lib().cvhip_mesh_merge(device.handle, _p(poly), _p(cam), len(poly), _p(out_p), _p(out_c), C.byref(n)),
               "cvhip_mesh_merge")
    return out_p[:n.value].copy(), out_c[:n.value].copy()


def create(device, surface, image_shapes, triangulate):
    """Mesh::create (:363-387) for a perspective surface: per camera the camera points, the caller's Delaunay
    `triangulate(xy [k, 2]) -> [f, 3]` (indices into xy; `delaunay_device(device)` needs no scipy), the culling, and the
    merged list.
    -> dict: polygons [p, 3] (track indices), camera [p], per_camera (points, polygons, kept, stats per camera)."""
    kept_p, kept_c, per_camera = [], [], []
    for i in range(len(surface.cameras)):
        index, xy = camera_points(device, surface, image_shapes, i)
        faces = np.asarray(triangulate(xy), dtype=np.int64).reshape(-1, 3)
        poly = index[faces].astype(np.uint32) if len(faces) else np.zeros((0, 3), dtype=np.uint32)
        keep, stats = cull(device, surface, image_shapes, i, poly)
        kept_p.append(poly[keep])
        kept_c.append(np.full(int(keep.sum()), i, dtype=np.uint32))
        per_camera.append({"points": len(index), "polygons": len(poly), "kept": int(keep.sum()), "stats": stats})
    polygons, camera = merge(device, np.concatenate(kept_p) if kept_p else np.zeros((0, 3), dtype=np.uint32),
                             np.concatenate(kept_c) if kept_c else np.zeros(0, dtype=np.uint32))
    return {"polygons": polygons, "camera": camera, "per_camera": per_camera}


def depth_image(device, surface, image_shapes, project_to_image: int, scale: float, polygons):
    """ImageWriter (:1016-1143) without the colour table and the encoder -> dict: map [height, width] f64 (NaN = None),
    origin (min_x, min_y), min_depth, max_depth, wide (polygons that took the wave path).  Raises CvhipError
    (CVHIP_ERR_NO_SURFACE, "No point projections found") when no projection is in range."""
    args, _keep = _surface_args(surface, image_shapes)
    poly = np.ascontiguousarray(polygons, dtype=np.uint32).reshape(-1, 3)
    w, h, wide = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    origin, minmax = np.zeros(2), np.zeros(2)
    L = _lib.lib()
    _lib.check(L.cvhip_mesh_depth_image(device.handle, *args, int(project_to_image), float(scale), _p(poly), len(poly), None, 0,
                                        C.byref(w), C.byref(h), _p(origin), None, None), "cvhip_mesh_depth_image")
    out = np.zeros((h.value, w.value))
    _lib.check(L.cvhip_mesh_depth_image(device.handle, *args, int(project_to_image), float(scale), _p(poly), len(poly), _p(out),
                                        out.size, C.byref(w), C.byref(h), _p(origin), _p(minmax), C.byref(wide)),
               "cvhip_mesh_depth_image")
    return {"map": out, "origin": (float(origin[0]), float(origin[1])), "min_depth": float(minmax[0]),
            "max_depth": float(minmax[1]), "wide": int(wide.value)}


def _image_args(images):
    """(images, image_offsets, image_dims) of cvhip_mesh_ply from a list of [h, w, 3] uint8 arrays, and the arrays kept alive."""
    imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
    if any(im.ndim != 3 or im.shape[2] != 3 for im in imgs):
        raise ValueError("images are [height, width, 3] uint8")
    flat = np.concatenate([im.reshape(-1) for im in imgs]) if imgs else np.zeros(0, dtype=np.uint8)
    offsets = np.zeros(len(imgs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([im.size for im in imgs], dtype=np.uint64)
    dims = np.array([[im.shape[1], im.shape[0]] for im in imgs], dtype=np.uint32).reshape(-1, 2)
    one = np.zeros(1, dtype=np.uint8)  # (an address for an empty array: the library reports what is wrong)
    return [C.c_void_p((flat if flat.size else one).ctypes.data), _p(offsets), _p(dims)], (flat, offsets, dims, one)


def _writer_args(surface, polygons, out_scale, images):
    """(points, tracks [n, m, 2], polygons [p, 3], out_scale, m) as cvhip_mesh_ply and cvhip_mesh_obj take them."""
    pts = _surface_array(surface.points, np.float64).reshape(-1, 3)
    tracks = _surface_array(surface.tracks, np.int32)
    if tracks.ndim != 3:
        tracks = tracks.reshape(len(pts), -1, 2)
    poly = np.ascontiguousarray(polygons, dtype=np.uint32).reshape(-1, 3)
    scale = np.array([float(v) for v in out_scale], dtype=np.float64)
    if scale.shape != (3,):
        raise ValueError("out_scale is (x, y, z)")
    m = tracks.shape[1]
    if images is not None and len(images) != m:
        raise ValueError("one image per image of a track")
    return pts, tracks, poly, scale, m


def _size_then_fill(name, args, *tail):
    """The entry `name` twice: `(*args, NULL, 0, &size, *tail)` for the size, then into an array of that size -> the array."""
    fn, size = getattr(_lib.lib(), name), C.c_uint64(0)
    _lib.check(fn(*args, None, 0, C.byref(size), *tail), name)
    out = np.zeros(size.value, dtype=np.uint8)
    _lib.check(fn(*args, _p(out), out.size, C.byref(size), *tail), name)
    return out


def _file_image(name, args, n_sections, sections):
    """_size_then_fill for a file image; `sections`, a list or None, receives its n_sections byte counts."""
    sec = np.zeros(n_sections, dtype=np.uint64)
    out = _size_then_fill(name, args, _p(sec))
    if sections is not None:
        sections[:] = [int(v) for v in sec]
    return out


def ply(device, surface, polygons, images=None, vertex_mode=VertexMode.Plain, out_scale=(1.0, 1.0, 1.0), sections=None):
    """The binary PLY file image of Mesh::output with a PlyWriter (output.rs:521-559, 648-772; cvhip_mesh_ply) -> uint8 array.
    images: one [h, w, 3] uint8 array per image of a track (Color mode only; a vertex takes the pixel of its track's first
    point, and no colour bytes when that point lies past its image).  `sections`, a list, receives the header's, the
    vertices' and the faces' byte counts.  Raises CvhipError ("Track has no images") for a track without a point in Color
    mode."""
    pts, tracks, poly, scale, m = _writer_args(surface, polygons, out_scale, images)
    img_args, _keep = _image_args(images) if images is not None else ([None, None, None], None)
    args = [device.handle, _p(pts), _p(tracks), len(pts), m, *img_args, int(vertex_mode), _p(scale), _p(poly), len(poly)]
    return _file_image("cvhip_mesh_ply", args, 3, sections)


def write_ply(path, device, surface, polygons, images=None, vertex_mode=VertexMode.Plain, out_scale=(1.0, 1.0, 1.0)):
    """`ply` written to `path` -> (header, vertex, face) byte counts."""
    sections = []
    ply(device, surface, polygons, images, vertex_mode, out_scale, sections=sections).tofile(path)
    return tuple(sections)


def _dims_args(dims):
    """(NULL, NULL, image_dims) of cvhip_mesh_obj from (width, height) pairs: Texture mode reads no pixels."""
    d = np.ascontiguousarray(np.asarray(dims, dtype=np.uint32).reshape(-1, 2))
    return [None, None, _p(d)], (d,)


def obj(device, surface, polygons, camera, images=None, vertex_mode=VertexMode.Plain, out_scale=(1.0, 1.0, 1.0), stem="mesh", sections=None):
    """The Wavefront OBJ file image of Mesh::output with an ObjWriter (output.rs:521-559, 774-1007; cvhip_mesh_obj) -> uint8 array.
    Every number is Rust's `{}`: the shortest decimal text that reads back as the same double, without an exponent.
    camera: the camera of each polygon ([p], mesh.create's "camera"; read in Texture mode: a usemtl line where it changes, and
    the uv index of a vertex counts the track's points in the images below it).  images: one [h, w, 3] uint8 array per image of
    a track (Color: a vertex takes the pixel of its track's first point / 255, and none when that point lies past its image;
    Texture: only the sizes are read, so a list of (width, height) does as well).  stem: the output's file stem (Texture:
    "mtllib {stem}.mtl").  `sections`, a list, receives the header's, the v, the vt and the f bytes.  Raises CvhipError ("Track
    has no images") for a track without a point in Color and Texture mode."""
    pts, tracks, poly, scale, m = _writer_args(surface, polygons, out_scale, images)
    cam = np.ascontiguousarray(camera if camera is not None else np.zeros(len(poly)), dtype=np.uint32).reshape(-1)
    if len(cam) != len(poly):
        raise ValueError("one camera per polygon")
    if images is None:
        img_args, _keep = [None, None, None], None
    elif all(hasattr(im, "shape") and len(im.shape) == 3 for im in images) and int(vertex_mode) != VertexMode.Texture:
        img_args, _keep = _image_args(images)
    else:
        img_args, _keep = _dims_args([(im.shape[1], im.shape[0]) if hasattr(im, "shape") else im for im in images])
    args = [device.handle, _p(pts), _p(tracks), len(pts), m, *img_args, int(vertex_mode), _p(scale), _p(poly), _p(cam), len(poly),
            str(stem).encode("utf-8")]
    return _file_image("cvhip_mesh_obj", args, 4, sections)


def obj_mtl(stem, m: int):
    """The {stem}.mtl text of ObjWriter::write_materials (output.rs:856-868; cvhip_mesh_obj_mtl) for m images -> bytes."""
    return _size_then_fill("cvhip_mesh_obj_mtl", [str(stem).encode("utf-8"), int(m)]).tobytes()


def write_obj(path, device, surface, polygons, camera, images=None, vertex_mode=VertexMode.Plain, out_scale=(1.0, 1.0, 1.0),
              save_textures=False):
    """`obj` written to `path` with the path's file stem and, in Texture mode, `obj_mtl` to {stem}.mtl next to it
    -> (header, v, vt, f) byte counts.  The .mtl names {stem}-{i}.png for image i: with save_textures, in Texture mode and with
    `images` given as arrays, `png` of image i is written there (ObjWriter::write_materials' img.save, output.rs:845-875)."""
    import pathlib

    path = pathlib.Path(path)
    sections = []
    obj(device, surface, polygons, camera, images, vertex_mode, out_scale, stem=path.stem, sections=sections).tofile(path)
    if int(vertex_mode) == VertexMode.Texture:
        m = _surface_array(surface.tracks, np.int32).reshape(len(surface.points), -1, 2).shape[1] if len(surface.points) else len(images or [])
        (path.parent / (path.stem + ".mtl")).write_bytes(obj_mtl(path.stem, m))
        if save_textures:
            write_obj_textures(path, device, images)
    return tuple(sections)


def write_obj_textures(obj_path, device, images):
    """The {stem}-{i}.png files that the .mtl of the OBJ at obj_path names: `png` of image i, for `images` given as arrays
    (nothing for a list of sizes, or None) -> the paths written."""
    import pathlib

    path, written = pathlib.Path(obj_path), []
    if images is None or not all(hasattr(im, "shape") and len(im.shape) == 3 for im in images):
        return written
    for i, im in enumerate(images):
        written.append(path.parent / ("%s-%d.png" % (path.stem, i)))
        write_png(written[-1], device, np.ascontiguousarray(im, dtype=np.uint8))  # (as _image_args takes them)
    return written


def f64_display(device, values):
    """Rust's `{}` of each double, formatted on the device (cvhip_f64_display) -> list of str."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    offsets = np.zeros(len(v) + 1, dtype=np.uint64)  # (the sizing call of values with text leaves it alone)
    text = _size_then_fill("cvhip_f64_display", [device.handle, _p(v), len(v)], _p(offsets)).tobytes().decode("ascii")
    return [text[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


def _table(table):
    t = np.ascontiguousarray(table, dtype=np.uint8)
    if t.shape != (256, 3):
        raise ValueError("the colour table is [256, 3] uint8: R, G, B per entry")
    return t


def colour_map(device, depth_map, min_depth: float, max_depth: float, table):
    """ImageWriter::complete's colour mapping (output.rs:1117-1229; cvhip_mesh_colour_map) of a depth map ([h, w] f64, NaN =
    None) -> [h, w, 4] uint8 RGBA.  table: [256, 3] uint8 (none is shipped)."""
    depth = np.ascontiguousarray(depth_map, dtype=np.float64)
    if depth.ndim != 2:
        raise ValueError("the depth map is [height, width]")
    t = _table(table)
    h, w = depth.shape
    out = np.zeros((h, w, 4), dtype=np.uint8)
    _lib.check(_lib.lib().cvhip_mesh_colour_map(device.handle, _p(depth), w, h, float(min_depth), float(max_depth), _p(t), _p(out)),
               "cvhip_mesh_colour_map")
    return out


def depth_image_rgba(device, surface, image_shapes, project_to_image: int, scale: float, polygons, table):
    """ImageWriter with its colour mapping (:1016-1229): cvhip_mesh_depth_image into device memory, cvhip_mesh_colour_map on
    it; only the RGBA crosses to the host -> dict: rgba [h, w, 4] uint8, origin, min_depth, max_depth."""
    import torch

    args, _keep = _surface_args(surface, image_shapes)
    poly = np.ascontiguousarray(polygons, dtype=np.uint32).reshape(-1, 3)
    t = _table(table)
    w, h = C.c_uint64(0), C.c_uint64(0)
    origin, minmax = np.zeros(2), np.zeros(2)
    L = _lib.lib()
    _lib.check(L.cvhip_mesh_depth_image(device.handle, *args, int(project_to_image), float(scale), _p(poly), len(poly), None, 0,
                                        C.byref(w), C.byref(h), _p(origin), None, None), "cvhip_mesh_depth_image")
    ordinal = getattr(device, "ordinal", -1)
    d_map = torch.empty((h.value, w.value), dtype=torch.float64, device=torch.device("cuda", ordinal) if ordinal >= 0 else "cuda")
    _lib.check(L.cvhip_mesh_depth_image(device.handle, *args, int(project_to_image), float(scale), _p(poly), len(poly),
                                        C.c_void_p(d_map.data_ptr()), d_map.numel(), C.byref(w), C.byref(h), _p(origin), _p(minmax),
                                        None), "cvhip_mesh_depth_image")
    rgba = np.zeros((h.value, w.value, 4), dtype=np.uint8)
    _lib.check(L.cvhip_mesh_colour_map(device.handle, C.c_void_p(d_map.data_ptr()), w.value, h.value, float(minmax[0]),
                                       float(minmax[1]), _p(t), _p(rgba)), "cvhip_mesh_colour_map")
    return {"rgba": rgba, "origin": (float(origin[0]), float(origin[1])), "min_depth": float(minmax[0]),
            "max_depth": float(minmax[1])}


class PngFilter(enum.IntEnum):
    """The `filter` of cvhip_png_encode (CVHIP_PNG_FILTER_*): one PNG filter on every row, or per row the one of least sum of
    |signed byte|."""
    Nothing = 0
    Sub = 1
    Up = 2
    Average = 3
    Paeth = 4
    Adaptive = 5


def _pixel_args(pixels):
    """(pixels, width, height, channels) of cvhip_png_encode from [h, w] or [h, w, c] uint8, as numpy or as a device tensor, and
    what keeps the memory alive."""
    if hasattr(pixels, "data_ptr"):  # a torch tensor
        import torch

        t = pixels.contiguous()
        if t.dtype != torch.uint8:
            raise ValueError("pixels are uint8")
        if t.is_cuda:
            torch.cuda.current_stream(t.device).synchronize()  # (filled on torch's stream; the library works on its own)
        shape, ptr, keep = tuple(t.shape), C.c_void_p(t.data_ptr()), t
    else:
        a = np.ascontiguousarray(pixels)
        if a.dtype != np.uint8:
            raise ValueError("pixels are uint8")
        shape, ptr, keep = a.shape, C.c_void_p(a.ctypes.data), a
    if len(shape) == 2:
        shape = (*shape, 1)
    if len(shape) != 3:
        raise ValueError("pixels are [height, width] or [height, width, channels]")
    return [ptr, int(shape[1]), int(shape[0]), int(shape[2])], keep


def png(device, pixels, filter=PngFilter.Adaptive, sections=None):
    """The PNG file image of an 8-bit image (cvhip_png_encode) -> uint8 array.  pixels: [h, w] or [h, w, c]
    uint8 with c = 1 (grey), 2 (grey and alpha), 3 (RGB) or 4 (RGBA), as a numpy array or as a device tensor (then they do
    not leave the device).  filter: a PngFilter.  `sections`, a list, receives the bytes before the IDAT data, the IDAT
    data's, and the bytes after it.  Any PNG decoder returns `pixels`; the bytes themselves are defined by this library."""
    args, _keep = _pixel_args(pixels)
    return _file_image("cvhip_png_encode", [device.handle, *args, int(filter)], 3, sections)


def write_png(path, device, pixels, filter=PngFilter.Adaptive):
    """`png` written to `path` -> (before, IDAT data, after) byte counts."""
    sections = []
    png(device, pixels, filter, sections=sections).tofile(path)
    return tuple(sections)


def _depth_rgba_device(device, surface, image_shapes, project_to_image, scale, polygons, table):
    """depth_image_rgba's two calls with the map AND the RGBA in device memory -> (rgba tensor [h, w, 4], origin, minmax)."""
    import torch

    args, _keep = _surface_args(surface, image_shapes)
    poly = np.ascontiguousarray(polygons, dtype=np.uint32).reshape(-1, 3)
    t = _table(table)
    w, h = C.c_uint64(0), C.c_uint64(0)
    origin, minmax = np.zeros(2), np.zeros(2)
    L = _lib.lib()
    _lib.check(L.cvhip_mesh_depth_image(device.handle, *args, int(project_to_image), float(scale), _p(poly), len(poly), None, 0,
                                        C.byref(w), C.byref(h), _p(origin), None, None), "cvhip_mesh_depth_image")
    ordinal = getattr(device, "ordinal", -1)
    where = torch.device("cuda", ordinal) if ordinal >= 0 else "cuda"
    d_map = torch.empty((h.value, w.value), dtype=torch.float64, device=where)
    d_rgba = torch.empty((h.value, w.value, 4), dtype=torch.uint8, device=where)
    _lib.check(L.cvhip_mesh_depth_image(device.handle, *args, int(project_to_image), float(scale), _p(poly), len(poly),
                                        C.c_void_p(d_map.data_ptr()), d_map.numel(), C.byref(w), C.byref(h), _p(origin), _p(minmax),
                                        None), "cvhip_mesh_depth_image")
    _lib.check(L.cvhip_mesh_colour_map(device.handle, C.c_void_p(d_map.data_ptr()), w.value, h.value, float(minmax[0]),
                                       float(minmax[1]), _p(t), C.c_void_p(d_rgba.data_ptr())), "cvhip_mesh_colour_map")
    return d_rgba, origin, minmax


def write_depth_png(path, device, surface, image_shapes, project_to_image: int, scale: float, polygons, table,
                    filter=PngFilter.Adaptive):
    """ImageWriter::complete with its img.save (output.rs:1016-1229, 1141): cvhip_mesh_depth_image, cvhip_mesh_colour_map and
    cvhip_png_encode chained in device memory - neither the map nor the RGBA crosses to the host, only the file does -> dict:
    width, height, origin, min_depth, max_depth, sections.  The file decodes to depth_image_rgba(...)["rgba"]."""
    d_rgba, origin, minmax = _depth_rgba_device(device, surface, image_shapes, project_to_image, scale, polygons, table)
    sections = write_png(path, device, d_rgba, filter)
    return {"width": int(d_rgba.shape[1]), "height": int(d_rgba.shape[0]), "origin": (float(origin[0]), float(origin[1])),
            "min_depth": float(minmax[0]), "max_depth": float(minmax[1]), "sections": sections}


class JpegSampling(enum.IntEnum):
    """The `sampling` of cvhip_jpeg_encode (CVHIP_JPEG_SAMPLING_*, Pillow's subsampling numbers): the luma blocks of an MCU
    over one block of each chroma component."""
    S444 = 0
    S422 = 1
    S420 = 2


JPEG_ENCODE_STATS = ("blocks", "dummy_blocks", "bits", "stuffed")


def jpeg(device, pixels, quality=75, sampling=JpegSampling.S420, optimize=False, sections=None):
    """The baseline JPEG file image of an 8-bit image (cvhip_jpeg_encode) -> uint8 array: the file that
    libjpeg writes at this quality (1 .. 100), sampling (a JpegSampling; a grey image ignores it) and with the Annex K Huffman
    tables or, with optimize, its optimal ones.  pixels: [h, w] or [h, w, c] uint8 with c = 1 (grey), 2 (grey and alpha), 3
    (RGB) or 4 (RGBA), as a numpy array or as a device tensor (then they do not leave the device); alpha is dropped.
    `sections`, a list, receives the bytes before the scan's data, the data's, and the bytes after it."""
    args, _keep = _pixel_args(pixels)
    return _file_image("cvhip_jpeg_encode", [device.handle, *args, int(quality), int(sampling), int(bool(optimize))], 3, sections)


def jpeg_encode_last_stats() -> dict:
    """cvhip_jpeg_encode_last_stats: of this thread's last `jpeg` - blocks, dummy blocks (luma blocks of an edge MCU beyond the
    image), the bits of the data before padding and stuffing, the zero bytes stuffed in."""
    s = np.zeros(len(JPEG_ENCODE_STATS), dtype=np.uint64)
    _lib.check(_lib.lib().cvhip_jpeg_encode_last_stats(C.c_void_p(s.ctypes.data)), "cvhip_jpeg_encode_last_stats")
    return dict(zip(JPEG_ENCODE_STATS, (int(v) for v in s)))


def write_jpeg(path, device, pixels, quality=75, sampling=JpegSampling.S420, optimize=False):
    """`jpeg` written to `path` -> (before, scan data, after) byte counts."""
    sections = []
    jpeg(device, pixels, quality, sampling, optimize, sections=sections).tofile(path)
    return tuple(sections)


def write_depth_jpeg(path, device, surface, image_shapes, project_to_image: int, scale: float, polygons, table, quality=75,
                     sampling=JpegSampling.S420, optimize=False):
    """write_depth_png with cvhip_jpeg_encode as the encoder: the depth map's RGBA stays in device memory, only the file
    crosses -> dict: width, height, origin, min_depth, max_depth, sections.  The file is that of the RGB of
    depth_image_rgba(...)["rgba"]: alpha is dropped, a cell without a depth is black."""
    d_rgba, origin, minmax = _depth_rgba_device(device, surface, image_shapes, project_to_image, scale, polygons, table)
    sections = write_jpeg(path, device, d_rgba, quality, sampling, optimize)
    return {"width": int(d_rgba.shape[1]), "height": int(d_rgba.shape[0]), "origin": (float(origin[0]), float(origin[1])),
            "min_depth": float(minmax[0]), "max_depth": float(minmax[1]), "sections": sections}


class TiffCompression(enum.IntEnum):
    """The `compression` of cvhip_tiff_encode (CVHIP_TIFF_COMPRESSION_*, the values of TIFF's tag 259)."""
    NONE = 1
    LZW = 5
    PACKBITS = 32773


TIFF_ENCODE_STATS = ("strips", "codes", "clears", "packets")


def tiff(device, pixels, compression=TiffCompression.LZW, predictor=None, rows_per_strip=0, sections=None):
    """The classic little-endian TIFF file image of an 8-bit image (cvhip_tiff_encode) -> uint8 array.
    pixels: [h, w] or [h, w, c] uint8 with c = 1 (grey), 2 (grey and alpha), 3 (RGB) or 4 (RGBA), as a numpy array or as a
    device tensor (then they do not leave the device).  compression: a TiffCompression; the LZW strips are libtiff's byte for
    byte.  predictor: 1 or 2 (horizontal differencing, with LZW only); None - 2 with LZW, 1 otherwise.  rows_per_strip: 0 -
    about 8 KB a strip.  `sections`, a list, receives the bytes before the first strip, the strips' with their padding, and
    the bytes after (0)."""
    args, _keep = _pixel_args(pixels)
    if predictor is None:
        predictor = 2 if int(compression) == TiffCompression.LZW else 1
    return _file_image("cvhip_tiff_encode", [device.handle, *args, int(compression), int(predictor), int(rows_per_strip)], 3, sections)


def tiff_encode_last_stats() -> dict:
    """cvhip_tiff_encode_last_stats: of this thread's last `tiff` - strips, LZW codes (Clears and EOIs included), Clear codes,
    PackBits packets."""
    s = np.zeros(len(TIFF_ENCODE_STATS), dtype=np.uint64)
    _lib.check(_lib.lib().cvhip_tiff_encode_last_stats(C.c_void_p(s.ctypes.data)), "cvhip_tiff_encode_last_stats")
    return dict(zip(TIFF_ENCODE_STATS, (int(v) for v in s)))


def write_tiff(path, device, pixels, compression=TiffCompression.LZW, predictor=None, rows_per_strip=0):
    """`tiff` written to `path` -> (before, strips, after) byte counts."""
    sections = []
    tiff(device, pixels, compression, predictor, rows_per_strip, sections=sections).tofile(path)
    return tuple(sections)


def write_depth_tiff(path, device, surface, image_shapes, project_to_image: int, scale: float, polygons, table,
                     compression=TiffCompression.LZW, predictor=None, rows_per_strip=0):
    """write_depth_png with cvhip_tiff_encode as the encoder: the depth map's RGBA stays in device memory, only the file
    crosses -> dict: width, height, origin, min_depth, max_depth, sections.  The file decodes to
    depth_image_rgba(...)["rgba"]: four samples, the fourth unassociated alpha."""
    d_rgba, origin, minmax = _depth_rgba_device(device, surface, image_shapes, project_to_image, scale, polygons, table)
    sections = write_tiff(path, device, d_rgba, compression, predictor, rows_per_strip)
    return {"width": int(d_rgba.shape[1]), "height": int(d_rgba.shape[0]), "origin": (float(origin[0]), float(origin[1])),
            "min_depth": float(minmax[0]), "max_depth": float(minmax[1]), "sections": sections}


def set_delaunay_lane_cells(device, cells: int):
    """cvhip_mesh_delaunay_set_lane_cells: a device star that would visit more than `cells` grid cells is finished on the
    exact host path (LANE_CELLS_HOST = 0: every star, LANE_CELLS_UNBOUNDED: none for its size).  The faces do not change."""
    _lib.check(_lib.lib().cvhip_mesh_delaunay_set_lane_cells(device.handle, int(cells)), "cvhip_mesh_delaunay_set_lane_cells")


def set_delaunay_lattice(device, on: bool):
    """cvhip_mesh_delaunay_set_lattice: with it on, a call whose coordinates are all integers within 2^24 (the camera points
    of an affine surface) builds its stars - exact ties included - on the device with exact integer predicates; any other
    call is not affected.  The faces do not change.  Off by default."""
    _lib.check(_lib.lib().cvhip_mesh_delaunay_set_lattice(device.handle, int(bool(on))), "cvhip_mesh_delaunay_set_lattice")


def delaunay_lattice(device) -> bool:
    """cvhip_mesh_delaunay_get_lattice: whether set_delaunay_lattice is on."""
    on = C.c_int(0)
    _lib.check(_lib.lib().cvhip_mesh_delaunay_get_lattice(device.handle, C.byref(on)), "cvhip_mesh_delaunay_get_lattice")
    return bool(on.value)


def delaunay_lattice_stars(device) -> int:
    """cvhip_mesh_delaunay_get_lattice_stars: the stars of the last `delaunay` call on this device that the lattice kernels
    finished; 0 when that call did not qualify."""
    n = C.c_uint64(0)
    _lib.check(_lib.lib().cvhip_mesh_delaunay_get_lattice_stars(device.handle, C.byref(n)), "cvhip_mesh_delaunay_get_lattice_stars")
    return int(n.value)


def delaunay(device, xy, stats=None):
    """cvhip_mesh_delaunay: the Delaunay triangulation of the distinct positions of xy ([k, 2] f64) -> [f, 3] uint32 faces,
    counter-clockwise, the smallest index first, grouped by it; exact ties are fanned from their lowest index, of several
    indices at one position the lowest is the vertex (include/cvhip.h has the definition).  `stats`, a dict, receives
    DELAUNAY_STATS.  Raises CvhipError for a coordinate that is not finite."""
    pts = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    k = len(pts)
    faces = np.zeros((2 * k, 3), dtype=np.uint32)  # (2 k faces are always enough: one call, no sizing pass)
    n, st = C.c_uint64(0), np.zeros(len(DELAUNAY_STATS), dtype=np.uint64)
    _lib.check(_lib.lib().cvhip_mesh_delaunay(device.handle, _p(pts), k, _p(faces), len(faces), C.byref(n), _p(st)), "cvhip_mesh_delaunay")
    if stats is not None:
        stats.update(zip(DELAUNAY_STATS, (int(v) for v in st)))
    return faces[:n.value].copy()


def delaunay_device(device, lattice=None):
    """A `triangulate` for `create` and reconstruct_perspective_mesh(triangulate=...) that runs on the device (`delaunay`):
    the way to build a mesh without scipy.  lattice: True / False - set_delaunay_lattice for the length of each call (the
    device's setting is put back after it); None - the device's setting as it is."""
    def triangulate(xy):
        if lattice is None:
            return delaunay(device, xy)
        before = delaunay_lattice(device)
        set_delaunay_lattice(device, lattice)
        try:
            return delaunay(device, xy)
        finally:
            set_delaunay_lattice(device, before)

    return triangulate


def delaunay_scipy(xy):
    """A `triangulate` for `create`: scipy.spatial.Delaunay's simplices of the points ([k, 2] -> [f, 3]).  scipy is
    optional: without it this raises (the package itself does not need it; `delaunay_device` runs without it)."""
    try:
        from scipy.spatial import Delaunay
    except ImportError as exc:
        raise RuntimeError("delaunay_scipy needs scipy (scipy.spatial.Delaunay); pass another `triangulate` to "
                           "mesh.create, or install scipy") from exc
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    if len(xy) < 3:
        return np.zeros((0, 3), dtype=np.int64)
    return np.asarray(Delaunay(xy).simplices, dtype=np.int64)
