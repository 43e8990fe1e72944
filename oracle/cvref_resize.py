"""numpy restatement of image::imageops::resize(.., FilterType::Lanczos3) for Luma8 images, as SourceImage::resize
calls it (src/reconstruction.rs:146-162).  TEST INFRASTRUCTURE ONLY (see oracle/cvref.h).

The `image` crate (0.25.10, Cargo.lock:475-476) is a third-party dependency that is NOT vendored with the reference;
this follows its published algorithm (imageops/sample.rs: `resize` = `vertical_sample` into an f32 image, then
`horizontal_sample`; `lanczos3_kernel`, `sinc`), in float32 like the crate: one IEEE f32 operation per step, in the
crate's order.  The one step that is not an IEEE operation is the sine: it is the RUNNING MACHINE's libm `sinf`, called
through ctypes one argument at a time - what Rust's f32::sin resolves to on linux-gnu, and what the device's host-built
tables use (std::sin(float)).  numpy's own float32 sine is a SIMD kernel of numpy's and differs from libm's by one ulp on
about an eighth of the arguments met here, so it is not used.  Parity unpinned: no fixture of the reference holds a
resized image; but the device and this module perform the same operations on the same values, so the tests compare
their bytes by equality (tests/test_resize.py, MAX_DIFF = 0), and pin this module to an independent float64 statement of
the formula (tests/ref_resize.py).
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

F = np.float32

_libm = ctypes.CDLL("libm.so.6")
_libm.sinf.restype = ctypes.c_float
_libm.sinf.argtypes = [ctypes.c_float]


def sinf(a):
    """libm's sinf of every element of the f32 array `a` (a Python float holds an f32 exactly, both ways)."""
    a = np.asarray(a, dtype=F)
    f = _libm.sinf
    return np.array([f(v) for v in a.ravel().tolist()], dtype=F).reshape(a.shape)


def _sinc(t):
    a = t * F(np.pi)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(t == 0, F(1.0), sinf(a) / a).astype(F)


def lanczos3_kernel(x):
    x = np.asarray(x, dtype=F)
    return np.where(np.abs(x) < F(3.0), _sinc(x) * _sinc(x / F(3.0)), F(0.0)).astype(F)


def _raw_taps(in_size: int, out_size: int, o: int):
    """(left, f32 window values before normalisation) of output sample o."""
    ratio = F(in_size) / F(out_size)
    sratio = F(1.0) if ratio < F(1.0) else ratio
    src_support = F(3.0) * sratio
    centre = (F(o) + F(0.5)) * ratio
    left = int(np.floor(centre - src_support))
    left = min(max(left, 0), in_size - 1)
    right = int(np.ceil(centre + src_support))
    right = min(max(right, left + 1), in_size)
    centre = centre - F(0.5)
    return left, lanczos3_kernel((np.arange(left, right).astype(F) - centre) / sratio)


def _taps(in_size: int, out_size: int, o: int):
    """(left, normalised f32 weights) of output sample o."""
    left, w = _raw_taps(in_size, out_size, o)
    total = F(0.0)
    for v in w:            # `sum += w` in source order, f32
        total = F(total + v)
    return left, (w / total).astype(F)


@functools.lru_cache(maxsize=64)
def taps_of(in_size: int, out_size: int):
    """The taps of every output sample of one (in, out) pair, kept: a tuple of (left, weights)."""
    return tuple(_taps(in_size, out_size, o) for o in range(out_size))


def _sample_axis0(img_f32, out_size: int):
    """vertical_sample: [h, w] -> [out_size, w], f32 accumulation in tap order."""
    h, w = img_f32.shape
    out = np.zeros((out_size, w), dtype=F)
    for o, (left, ws) in enumerate(taps_of(h, out_size)):
        t = np.zeros(w, dtype=F)
        for i, wi in enumerate(ws):
            t = (t + img_f32[left + i] * wi).astype(F)
        out[o] = t
    return out


def resample_f32(img, nw: int, nh: int):
    """The two passes without the final clamp and rounding: [nh, nw] f32."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    tmp = _sample_axis0(img.astype(F), nh)                  # vertical pass, unclamped f32
    return _sample_axis0(np.ascontiguousarray(tmp.T), nw).T  # horizontal pass


def to_u8(out):
    out = np.clip(out, F(0.0), F(255.0))
    # FloatNearest -> f32::round (half away from zero); values are >= 0 here
    fl = np.floor(out)
    return (fl + ((out - fl) >= F(0.5))).astype(np.uint8)


def resize_lanczos3(img, nw: int, nh: int):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    if (nw, nh) == (w, h):
        return img.copy()
    return to_u8(resample_f32(img, nw, nh))


def resize_scale(img, scale: float):
    """SourceImage::resize (reconstruction.rs:146-152): dims = (w as f32 * scale) as u32."""
    h, w = img.shape
    return resize_lanczos3(img, int(F(w) * F(scale)), int(F(h) * F(scale)))
