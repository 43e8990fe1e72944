"""Image files in: what SourceImage::load / load_rgb do with a path (src/reconstruction.rs:39-60) - the
file's pixels as Luma8 or RGB8 with `databar_height` rows cut from the bottom, the EXIF FocalLengthIn35mmFilm (:138-142) -
and SourceImage::calibration_matrix (:164-185).  Baseline JPEG (cvhip_jpeg_decode): the host walks the markers, the
entropy decode, IDCT, upsampling and colour conversion run on the device.  Strip TIFF (cvhip_tiff_decode):
the host walks the IFD and reads the SEM text block of tag 34683 / 34682 - scale, tilt_angle, databar_height (:80-144) -,
LZW / PackBits decompression, Predictor 2 and the conversion run on the device.  PNG (cvhip_png_decode):
the host walks the chunks and reads IHDR, PLTE and the eXIf chunk's focal length, inflate, the IDAT CRCs, the Adler-32, the
five filters and the conversion run on the device; every colour type and bit depth, alpha and tRNS dropped, the SEM fields
keep their defaults.  Progressive JPEG (cvhip_jpeg_progressive_decode): the host walks the markers of the
whole file and checks the progression, the entropy decode of every scan accumulates the coefficients on the device, the tail
is the baseline path's; `load` takes it for a file whose first SOF marker is SOF2.  Deflate and tiled TIFF (DESIGN.md 4.23;
cvhip_tiff_ext_decode): the host walk also reads the tile tags, inflate runs a workgroup per strip or tile, the tiles go through
the strip decompressors, the conversion gathers a row from its tiles; `load` takes it for a TIFF file with a tile tag or
compression 8 / 32946.  Adam7 interlaced PNG (cvhip_png_ext_decode): the stream's seven reduced images are
unfiltered side by side and interleaved by the conversion; `load` takes it for a PNG file whose IHDR says interlace method 1.
Of JPEG arithmetic coding, 12 bits, sequential files of several scans and incomplete progressions are not built."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _lib

LUMA8, RGB8 = 0, 1  # CVHIP_IMAGE_LUMA8, CVHIP_IMAGE_RGB8
TIFF_DROP_DATABAR = 0xFFFFFFFF  # CVHIP_TIFF_DROP_DATABAR
_MODES = {"L": LUMA8, "RGB": RGB8}


def _file(data):
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    one = np.zeros(1, dtype=np.uint8)  # (an address for an empty file: the library reports what is wrong)
    return C.c_void_p((buf if buf.size else one).ctypes.data), int(buf.size), (buf, one)


def jpeg_info(data) -> dict:
    """cvhip_jpeg_info of a file's bytes (host only) -> width, height, components, h, v (the luma sampling factors) and
    focal_length_35mm (None when the file has none)."""
    p, n, _keep = _file(data)
    info = np.zeros(6, dtype=np.uint32)
    _lib.check(_lib.lib().cvhip_jpeg_info(p, n, C.c_void_p(info.ctypes.data)), "cvhip_jpeg_info")
    w, h, comps, hs, vs, focal = (int(v) for v in info)
    return {"width": w, "height": h, "components": comps, "h": hs, "v": vs, "focal_length_35mm": focal or None}


def _decode(name, device, data, mode, drop_rows, out, width_of):
    """The sizing call, the buffer and the filling call of cvhip_jpeg_decode / cvhip_tiff_decode / cvhip_png_decode; width_of(data): the
    image's width, asked once the sizing call has accepted the file."""
    if mode not in _MODES:
        raise ValueError('mode is "L" or "RGB"')
    p, n, _keep = _file(data)
    call = getattr(_lib.lib(), name)
    size = C.c_uint64(0)
    _lib.check(call(device.handle, p, n, _MODES[mode], int(drop_rows), None, 0, C.byref(size)), name)
    width = width_of(data)
    shape = (size.value // (width * (3 if mode == "RGB" else 1)), width) + ((3,) if mode == "RGB" else ())
    if out is None:
        out = np.empty(shape, dtype=np.uint8)
    elif isinstance(out, str):
        if out != "device":
            raise ValueError('out is None, "device", an array or a tensor')
        import torch

        ordinal = getattr(device, "ordinal", -1)
        out = torch.empty(shape, dtype=torch.uint8, device=torch.device("cuda", ordinal) if ordinal >= 0 else "cuda")
    if hasattr(out, "data_ptr"):
        ptr, cap = C.c_void_p(out.data_ptr()), out.numel() * out.element_size()
    else:
        ptr, cap = C.c_void_p(out.ctypes.data), out.nbytes
    _lib.check(call(device.handle, p, n, _MODES[mode], int(drop_rows), ptr, cap, C.byref(size)), name)
    return out


def decode_jpeg(device, data, mode: str = "L", drop_rows: int = 0, out=None):
    """cvhip_jpeg_decode of a file's bytes -> [height - drop_rows, width] (mode "L") or [.., .., 3] (mode "RGB") uint8.
    out: None - a numpy array; "device" - a torch tensor on the device; or the numpy array / device tensor to fill (its
    first bytes; it is returned as given)."""
    return _decode("cvhip_jpeg_decode", device, data, mode, drop_rows, out, lambda d: jpeg_info(d)["width"])


def jpeg_progressive_info(data) -> dict:
    """cvhip_jpeg_progressive_info of a file's bytes (host only) -> jpeg_info's fields and scans, the number of scans."""
    p, n, _keep = _file(data)
    info = np.zeros(7, dtype=np.uint32)
    _lib.check(_lib.lib().cvhip_jpeg_progressive_info(p, n, C.c_void_p(info.ctypes.data)), "cvhip_jpeg_progressive_info")
    w, h, comps, hs, vs, focal, scans = (int(v) for v in info)
    return {"width": w, "height": h, "components": comps, "h": hs, "v": vs, "focal_length_35mm": focal or None, "scans": scans}


def decode_jpeg_progressive(device, data, mode: str = "L", drop_rows: int = 0, out=None):
    """cvhip_jpeg_progressive_decode of a progressive file's bytes, as decode_jpeg."""
    return _decode("cvhip_jpeg_progressive_decode", device, data, mode, drop_rows, out, lambda d: jpeg_progressive_info(d)["width"])


def jpeg_progressive_last_stats() -> dict:
    """cvhip_jpeg_progressive_last_stats: of this thread's last progressive decode - scans, restart intervals, subsequences,
    launches of the synchronisation kernel that settles the first scans, the most rounds a workgroup needed within a launch,
    AC-refinement scans, the launches that hold one, the longest EOB run."""
    s = np.zeros(8, dtype=np.uint64)
    _lib.check(_lib.lib().cvhip_jpeg_progressive_last_stats(C.c_void_p(s.ctypes.data)), "cvhip_jpeg_progressive_last_stats")
    names = ("scans", "intervals", "subsequences", "sync_launches", "workgroup_rounds", "ac_refinement_scans", "ac_refinement_launches", "longest_eob_run")
    return {k: int(v) for k, v in zip(names, s)}


def _first_sof(data) -> int:
    """The first SOFn marker of a JPEG file's segments (0xC0 .. 0xCF without DHT, JPG and DAC), 0 where the walk finds none."""
    n, at = len(data), 2
    if data[:2] != b"\xff\xd8":
        return 0
    while at + 4 <= n and data[at] == 0xFF:
        while at < n and data[at] == 0xFF:
            at += 1
        if at + 2 >= n:
            return 0
        m = data[at]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return m
        if m == 0xDA or m == 0xD9:
            return 0
        at += 1 + (0 if m == 0x01 or 0xD0 <= m <= 0xD7 else data[at + 1] << 8 | data[at + 2])
    return 0


def tiff_info(data) -> dict:
    """cvhip_tiff_info of a file's bytes (host only) -> width, height, samples, bits, compression, photometric, predictor,
    strips, rows_per_strip, focal_length_35mm (None when the file has none), databar_height, sem (a block was found),
    scale (width, height; 1.0 each by default) and tilt_angle (None when the block sets none)."""
    p, n, _keep = _file(data)
    info, scale = np.zeros(12, dtype=np.uint32), np.zeros(3, dtype=np.float32)
    _lib.check(_lib.lib().cvhip_tiff_info(p, n, C.c_void_p(info.ctypes.data), C.c_void_p(scale.ctypes.data)), "cvhip_tiff_info")
    names = ("width", "height", "samples", "bits", "compression", "photometric", "predictor", "strips", "rows_per_strip")
    out = {k: int(v) for k, v in zip(names, info)}
    out.update(focal_length_35mm=int(info[9]) or None, databar_height=int(info[10]), sem=bool(info[11] & 1), scale=(float(scale[0]), float(scale[1])),
               tilt_angle=float(scale[2]) if info[11] & 2 else None)
    return out


def decode_tiff(device, data, mode: str = "L", drop_rows=None, out=None):
    """cvhip_tiff_decode of a file's bytes, as decode_jpeg; drop_rows=None cuts the file's own DatabarHeight."""
    return _decode("cvhip_tiff_decode", device, data, mode, TIFF_DROP_DATABAR if drop_rows is None else drop_rows, out, lambda d: tiff_info(d)["width"])


def tiff_last_stats() -> dict:
    """cvhip_tiff_last_stats: of this thread's last decode - strips, LZW codes read, Clear codes met, the longest string."""
    s = np.zeros(4, dtype=np.uint64)
    _lib.check(_lib.lib().cvhip_tiff_last_stats(C.c_void_p(s.ctypes.data)), "cvhip_tiff_last_stats")
    return {"strips": int(s[0]), "codes": int(s[1]), "clears": int(s[2]), "longest": int(s[3])}


def tiff_ext_info(data) -> dict:
    """cvhip_tiff_ext_info of a file's bytes (host only) -> tiff_info's fields - of a tiled file strips is the number of tiles
    and rows_per_strip TileLength - and tile_width, tile_length, tiles_across (all 0 for a strip file)."""
    p, n, _keep = _file(data)
    info, scale = np.zeros(16, dtype=np.uint32), np.zeros(3, dtype=np.float32)
    _lib.check(_lib.lib().cvhip_tiff_ext_info(p, n, C.c_void_p(info.ctypes.data), C.c_void_p(scale.ctypes.data)), "cvhip_tiff_ext_info")
    names = ("width", "height", "samples", "bits", "compression", "photometric", "predictor", "strips", "rows_per_strip")
    out = {k: int(v) for k, v in zip(names, info)}
    out.update(focal_length_35mm=int(info[9]) or None, databar_height=int(info[10]), sem=bool(info[11] & 1), scale=(float(scale[0]), float(scale[1])),
               tilt_angle=float(scale[2]) if info[11] & 2 else None, tile_width=int(info[12]), tile_length=int(info[13]), tiles_across=int(info[14]))
    return out


def decode_tiff_ext(device, data, mode: str = "L", drop_rows=None, out=None):
    """cvhip_tiff_ext_decode of a file's bytes, as decode_tiff: what that takes, and Deflate and tiled files."""
    return _decode("cvhip_tiff_ext_decode", device, data, mode, TIFF_DROP_DATABAR if drop_rows is None else drop_rows, out, lambda d: tiff_ext_info(d)["width"])


def tiff_ext_last_stats() -> dict:
    """cvhip_tiff_ext_last_stats: of this thread's last decode - streams (strips or tiles), LZW codes read, Clear codes met, the
    longest string; stored, fixed and dynamic deflate blocks over all streams, subsequences, the most settle rounds one window
    needed, settle windows, rounds of the copy resolution."""
    s = np.zeros(12, dtype=np.uint64)
    _lib.check(_lib.lib().cvhip_tiff_ext_last_stats(C.c_void_p(s.ctypes.data)), "cvhip_tiff_ext_last_stats")
    names = ("streams", "codes", "clears", "longest", "stored_blocks", "fixed_blocks", "dynamic_blocks", "subsequences", "settle_rounds", "settle_windows",
             "copy_rounds")
    return {k: int(v) for k, v in zip(names, s)}


def _tiff_is_ext(data) -> bool:
    """A classic TIFF file whose first IFD holds a tile tag (322 .. 325) or Compression 8 / 32946; False where the walk ends early."""
    order = "little" if data[:2] == b"II" else "big"
    ifd = int.from_bytes(data[4:8], order)
    if ifd + 2 > len(data):
        return False
    for k in range(int.from_bytes(data[ifd:ifd + 2], order)):
        entry = data[ifd + 2 + 12 * k:ifd + 14 + 12 * k]
        if len(entry) < 12:
            return False
        tag, kind = int.from_bytes(entry[:2], order), int.from_bytes(entry[2:4], order)
        if 322 <= tag <= 325:
            return True
        if tag == 259 and kind in (3, 4) and int.from_bytes(entry[8:10] if kind == 3 else entry[8:12], order) in (8, 32946):
            return True
    return False


def png_info(data) -> dict:
    """cvhip_png_info of a file's bytes (host only) -> width, height, colour_type, bit_depth, interlace, idat_chunks,
    focal_length_35mm (the eXIf chunk's; None when the file has none), plte and trns (such a chunk was read)."""
    p, n, _keep = _file(data)
    info = np.zeros(8, dtype=np.uint32)
    _lib.check(_lib.lib().cvhip_png_info(p, n, C.c_void_p(info.ctypes.data)), "cvhip_png_info")
    names = ("width", "height", "colour_type", "bit_depth", "interlace", "idat_chunks")
    out = {k: int(v) for k, v in zip(names, info)}
    out.update(focal_length_35mm=int(info[6]) or None, plte=bool(info[7] & 1), trns=bool(info[7] & 2))
    return out


def decode_png(device, data, mode: str = "L", drop_rows: int = 0, out=None):
    """cvhip_png_decode of a file's bytes, as decode_jpeg."""
    return _decode("cvhip_png_decode", device, data, mode, drop_rows, out, lambda d: png_info(d)["width"])


def png_last_stats() -> dict:
    """cvhip_png_last_stats: of this thread's last decode - stored, fixed and dynamic deflate blocks, subsequences, the most
    settle rounds one window needed, settle windows, rounds of the copy resolution, row segments of the unfilter pass."""
    s = np.zeros(8, dtype=np.uint64)
    _lib.check(_lib.lib().cvhip_png_last_stats(C.c_void_p(s.ctypes.data)), "cvhip_png_last_stats")
    names = ("stored_blocks", "fixed_blocks", "dynamic_blocks", "subsequences", "settle_rounds", "settle_windows", "copy_rounds", "row_segments")
    return {k: int(v) for k, v in zip(names, s)}


def png_ext_info(data) -> dict:
    """cvhip_png_ext_info of a file's bytes (host only) -> png_info's fields; interlace is 0 or 1 (Adam7)."""
    p, n, _keep = _file(data)
    info = np.zeros(8, dtype=np.uint32)
    _lib.check(_lib.lib().cvhip_png_ext_info(p, n, C.c_void_p(info.ctypes.data)), "cvhip_png_ext_info")
    names = ("width", "height", "colour_type", "bit_depth", "interlace", "idat_chunks")
    out = {k: int(v) for k, v in zip(names, info)}
    out.update(focal_length_35mm=int(info[6]) or None, plte=bool(info[7] & 1), trns=bool(info[7] & 2))
    return out


def decode_png_ext(device, data, mode: str = "L", drop_rows: int = 0, out=None):
    """cvhip_png_ext_decode of a file's bytes, as decode_png: what that takes, and Adam7 interlaced files."""
    return _decode("cvhip_png_ext_decode", device, data, mode, drop_rows, out, lambda d: png_ext_info(d)["width"])


def png_ext_last_stats() -> dict:
    """cvhip_png_ext_last_stats: of this thread's last decode - png_last_stats' fields, the row segments counted over all
    passes, and passes, the non-empty ones (1 for a file that is not interlaced)."""
    s = np.zeros(10, dtype=np.uint64)
    _lib.check(_lib.lib().cvhip_png_ext_last_stats(C.c_void_p(s.ctypes.data)), "cvhip_png_ext_last_stats")
    names = ("stored_blocks", "fixed_blocks", "dynamic_blocks", "subsequences", "settle_rounds", "settle_windows", "copy_rounds", "row_segments", "passes")
    return {k: int(v) for k, v in zip(names, s)}


def jpeg_last_stats() -> dict:
    """cvhip_jpeg_last_stats: of this thread's last decode - restart intervals, subsequences, launches of the synchronisation
    kernel, the most rounds a workgroup needed within a launch."""
    s = np.zeros(4, dtype=np.uint64)
    _lib.check(_lib.lib().cvhip_jpeg_last_stats(C.c_void_p(s.ctypes.data)), "cvhip_jpeg_last_stats")
    return {"intervals": int(s[0]), "subsequences": int(s[1]), "sync_launches": int(s[2]), "workgroup_rounds": int(s[3])}


@dataclass
class SourceImage:
    """SourceImage (reconstruction.rs:28-37): img (Luma8), rgb (on request), the EXIF focal length, the file's name, and of
    a TIFF file's SEM block scale, tilt_angle and the databar_height that was cut (the defaults for every other file)."""
    img: object
    rgb: object
    focal_length_35mm: int | None
    filename: str
    scale: tuple = (1.0, 1.0)
    tilt_angle: float | None = None
    databar_height: int = 0

    def calibration_matrix(self, focal_length_35mm=None):
        h, w = int(self.img.shape[0]), int(self.img.shape[1])
        return calibration_matrix(w, h, focal_length_35mm if focal_length_35mm is not None else self.focal_length_35mm)


def load(device, path, rgb: bool = False, drop_rows=None, out=None) -> SourceImage:
    """SourceImage::load (and load_rgb with rgb=True) of a TIFF, PNG or JPEG file, told apart by the first four (TIFF) or
    eight (PNG) bytes (a PNG file whose IHDR says Adam7 gets the interlaced path; a TIFF file with a tile tag or Compression 8 / 32946 gets the Deflate-and-tiles path; anything else gets the JPEG path and its error; a JPEG file whose first SOF marker is SOF2 the progressive one).  drop_rows: the rows cut from the bottom; None - the
    file's own databar_height (the DatabarHeight of a TIFF file's SEM block; 0 for PNG and JPEG).  out: None or "device", as decode_jpeg takes
    it, for img; rgb is a numpy array."""
    data = Path(path).read_bytes()
    if data[:4] in (b"II*\0", b"MM\0*"):
        info_of, decode = (tiff_ext_info, decode_tiff_ext) if _tiff_is_ext(data) else (tiff_info, decode_tiff)   # every other file goes where it went
        info = info_of(data)
        img = decode(device, data, "L", drop_rows, out)
        colour = decode(device, data, "RGB", drop_rows) if rgb else None
        return SourceImage(img, colour, info["focal_length_35mm"], str(path), info["scale"], info["tilt_angle"],
                           info["databar_height"] if drop_rows is None else int(drop_rows))
    drop_rows = 0 if drop_rows is None else drop_rows
    if data[:8] == b"\x89PNG\r\n\x1a\n":
        adam7 = len(data) > 28 and data[28] == 1   # IHDR's interlace byte: every other file goes where it went
        info_of, decode = (png_ext_info, decode_png_ext) if adam7 else (png_info, decode_png)
        info = info_of(data)
        img = decode(device, data, "L", drop_rows, out)
        colour = decode(device, data, "RGB", drop_rows) if rgb else None
        return SourceImage(img, colour, info["focal_length_35mm"], str(path))
    if _first_sof(data) == 0xC2:   # progressive: every other file goes where it went
        info = jpeg_progressive_info(data)
        img = decode_jpeg_progressive(device, data, "L", drop_rows, out)
        colour = decode_jpeg_progressive(device, data, "RGB", drop_rows) if rgb else None
        return SourceImage(img, colour, info["focal_length_35mm"], str(path))
    info = jpeg_info(data)
    img = decode_jpeg(device, data, "L", drop_rows, out)
    colour = decode_jpeg(device, data, "RGB", drop_rows) if rgb else None
    return SourceImage(img, colour, info["focal_length_35mm"], str(path))


def calibration_matrix(width: int, height: int, focal_length_35mm=None) -> np.ndarray:
    """SourceImage::calibration_matrix (reconstruction.rs:164-185) in f64: the focal length scaled by the image's diagonal
    over the 24 x 36 mm frame's; None or 0 falls back to 1 (`.unwrap_or(1)`)."""
    diagonal_35mm = math.sqrt(24.0 * 24.0 + 36.0 * 36.0)
    w, h = float(width), float(height)
    diagonal = math.sqrt(w * w + h * h)
    focal = float(focal_length_35mm or 1) * diagonal / diagonal_35mm
    return np.array([[focal, 0.0, w / 2.0], [0.0, focal, h / 2.0], [0.0, 0.0, 1.0]], dtype=np.float64)
