"""An independent float64 statement of the separable Lanczos3 resize, for tests/test_resize.py.

The published formula in matrix form: out = R_v . img . R_h^T.  Row o of R (out_size x in_size) holds
lanczos3((i - ((o + 1/2) ratio - 1/2)) / max(ratio, 1)) for the source samples i of [left, right), left =
floor(centre - 3 max(ratio, 1)) and right = ceil(centre + 3 max(ratio, 1)) clamped into the source (at least one sample),
zero elsewhere, divided by the row's sum; lanczos3(x) = sinc(x) sinc(x / 3) inside |x| < 3 with numpy's normalised sinc.
All float64, no tap loop, and nothing shared with oracle/cvref_resize.py.
"""
import numpy as np


def resample_matrix(in_size: int, out_size: int):
    ratio = in_size / out_size
    sratio = max(ratio, 1.0)
    centre = (np.arange(out_size, dtype=np.float64) + 0.5) * ratio
    left = np.clip(np.floor(centre - 3.0 * sratio), 0, in_size - 1)
    right = np.minimum(np.maximum(np.ceil(centre + 3.0 * sratio), left + 1), in_size)
    i = np.arange(in_size, dtype=np.float64)[None, :]
    x = (i - (centre[:, None] - 0.5)) / sratio
    r = np.where(np.abs(x) < 3.0, np.sinc(x) * np.sinc(x / 3.0), 0.0)
    r = np.where((i >= left[:, None]) & (i < right[:, None]), r, 0.0)
    return r / r.sum(axis=1, keepdims=True)


def resample_f64(img, nw: int, nh: int):
    """[nh, nw] float64, before the clamp and the rounding."""
    img = np.asarray(img)
    h, w = img.shape
    return resample_matrix(h, nh) @ img.astype(np.float64) @ resample_matrix(w, nw).T


def to_u8(v):
    """Clamp to [0, 255], round half up."""
    return np.floor(np.clip(v, 0.0, 255.0) + 0.5).astype(np.uint8)


def resize_lanczos3(img, nw: int, nh: int):
    img = np.asarray(img)
    if img.shape == (nh, nw):
        return img.astype(np.uint8).copy()
    return to_u8(resample_f64(img, nw, nh))
