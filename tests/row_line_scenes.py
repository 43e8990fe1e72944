"""Scenes for the lean box walk's row table (box_body.inc; cvhip_ctx_set_row_lines): rectified pairs whose
epipolar lines are exactly horizontal, so that every pixel of an image row has the same line and the kernel may take it
from one table entry per row - and pairs that are almost that, where it must not.

The base pair is 320 x 288 value noise (synth.texture) with synth's small integer disparity along x: three levels, the
first pass at 80 x 72 and box launches at 160 x 144 and at 320 x 288.  A line through row v has its five stripes on the
rows floor(v - 2) .. floor(v + 2); where v - 2 and v + 2 lie on either side of a power of two (rows 14-17, 30-33, 62-65,
126-129, 254-257 for lines through the pixel's own row) the kernel cannot tell from the binade alone that the stripes
are consecutive rows (`closed` is false) and checks them one by one.  A scene may shift image 2 vertically, with F[8]
saying so: the lines then lie `shift` full-resolution rows above the pixel's row (below, seen from image 2), and with a
large shift they leave the image at the top rows.

`row_claims` derives from the oracle's last-level lines what a scene is made for; the GPU test asks the library's getter
whether the table was used."""
from __future__ import annotations

import numpy as np

from cybervision_amd import synth

KERNEL_SIZE = 5
CORRIDOR = 2  # affine projection: five stripes


def _pair(w1, h1, w2, h2, shift, seed):
    """img1 = T(x, y) on w1 x h1, img2(x, y) = T(x + d(x, y), y + shift) on w2 x h2: the pixel (x, y) of image 1 is found
    in image 2 on row y - shift."""
    xs1 = np.arange(w1, dtype=np.int64)[None, :]
    ys1 = np.arange(h1, dtype=np.int64)[:, None]
    xs2 = np.arange(w2, dtype=np.int64)[None, :]
    ys2 = np.arange(h2, dtype=np.int64)[:, None]
    d = synth.disparity(w2, h2)
    t1 = synth.texture(xs1, ys1, seed)
    t2 = synth.texture(xs2 + d, ys2 + shift + 0 * xs2, seed)
    return (np.ascontiguousarray(np.clip(t1, 0, 255).astype(np.uint8)),
            np.ascontiguousarray(np.clip(t2, 0, 255).astype(np.uint8)))


def _f_horizontal(shift=0.0, factor=1.0, f6=None, f2=None):
    """F_HORIZONTAL with the lines `shift` rows above the pixel's row (forward), times `factor` (-1 turns its zeros into
    -0.0); f6 / f2: the entries that make the line depend on x in the forward / reverse direction (the reverse pass runs
    on F transposed)."""
    F = np.array(synth.F_HORIZONTAL, dtype=np.float64)
    F[2, 2] = shift
    F = F * factor
    if f6 is not None:
        F[2, 0] = f6
    if f2 is not None:
        F[0, 2] = f2
    return F


F_VERTICAL = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])

# name -> dict(images=(w1, h1, w2, h2, shift, seed, transposed), F, used=(forward, reverse) the getter's answer,
#              route: how the levels are run)
BASE = (320, 288, 320, 288, 0, 61, False)
SCENES = {
    "horizontal": dict(images=BASE, F=_f_horizontal(), used=(True, True)),
    "negated": dict(images=BASE, F=_f_horizontal(factor=-1.0), used=(True, True)),
    "scaled_1e-3": dict(images=BASE, F=_f_horizontal(factor=1e-3), used=(True, True)),
    "three_rows_off": dict(images=(320, 288, 320, 288, 3, 62, False), F=_f_horizontal(shift=3.0), used=(True, True)),
    "leaves_at_top": dict(images=(320, 288, 320, 288, 12, 63, False), F=_f_horizontal(shift=12.0), used=(True, True)),
    "f6_minus_zero": dict(images=BASE, F=_f_horizontal(f6=-0.0, f2=-0.0), used=(True, True)),
    # forward: lean launch, the line moves along the row - refused; reverse: F[2] of the transposed matrix is not zero - stepped
    "f6_1e-12": dict(images=BASE, F=_f_horizontal(f6=1e-12), used=(False, False)),
    # the other way round: forward stepped, reverse a lean launch whose table is refused
    "f2_1e-12": dict(images=BASE, F=_f_horizontal(f2=1e-12), used=(False, False)),
    "tilt3": dict(images=BASE, F=np.asarray(synth.f_tilt(3.0), dtype=np.float64), used=(False, False)),
    # vertical lines: the transposed lean launch, which keeps evaluating its lines per lane
    "vertical": dict(images=(320, 288, 320, 288, 0, 64, True), F=F_VERTICAL, used=(False, False)),
    "four_calls": dict(images=BASE, F=_f_horizontal(), used=(True, True), route=dict(fused=False)),
    "row_band_1_of_3": dict(images=BASE, F=_f_horizontal(), used=(True, True), route=dict(band=(1, 3))),
    "row_band_2_of_3": dict(images=BASE, F=_f_horizontal(), used=(True, True), route=dict(band=(2, 3))),
    "result_bands_3": dict(images=BASE, F=_f_horizontal(), used=(True, True), route=dict(result_bands=3)),
    "wider_352x288": dict(images=(320, 288, 352, 288, 0, 65, False), F=_f_horizontal(), used=(True, True)),
    "fold_off": dict(images=BASE, F=_f_horizontal(), used=(True, True), route=dict(fold=False)),
}


def make_scene(name):
    """name -> dict(name, img1, img2, F, projection, steps, used, route), as cases.make_case.  Deterministic."""
    s = SCENES[name]
    w1, h1, w2, h2, shift, seed, transposed = s["images"]
    a, b = _pair(w1, h1, w2, h2, shift, seed)
    if transposed:
        a, b = np.ascontiguousarray(a.T), np.ascontiguousarray(b.T)
    return dict(name=name, img1=a, img2=b, F=np.asarray(s["F"], dtype=np.float64), projection=0,
                steps=synth.optimal_scale_steps(a.shape[1], a.shape[0]), used=s["used"], route=dict(s.get("route", {})))


def image_key(name):
    """Scenes with the same images and F share one oracle run."""
    s = SCENES[name]
    return s["images"], s["F"].tobytes()


def pyramids(c):
    return synth.box_pyramid(c["img1"], c["steps"]), synth.box_pyramid(c["img2"], c["steps"])


def oracle_last_lines(oracle, c):
    """Per direction: the oracle's last-level search ranges [h, w, 2] (-1: not searched) and lines [h, w, 4] = (coeff_x,
    coeff_y, add_x, add_y)."""
    p1, p2 = pyramids(c)
    h1, w1 = c["img1"].shape
    h2, w2 = c["img2"].shape
    oc = oracle.Corr((w1, h1), (w2, h2), c["F"], c["projection"], 8)
    try:
        oc.export_ranges(0)
        oc.export_ranges(1)
        for i in range(c["steps"] + 1):
            k = c["steps"] - i
            oc.correlate_images(p1[k], p2[k], 1.0 / float(1 << k))
        return [oc.ranges(0, w1, h1), oc.ranges(1, w2, h2)]
    finally:
        oc.close()


def row_claims(ranges, lines):
    """What one direction's last level gives the lean kernel's setup, from the oracle's lines of the searched pixels:
    dict(row_major: every line runs along x with coeff_x = 1, add_x = 0; horizontal: coeff_y = +-0 everywhere;
    uniform: every searched pixel of a row has the same add_y; rows: {y: add_y} of the rows with a searched pixel;
    open: the rows whose stripes the binade rule does not settle (`closed` false); outside: the rows with m0 < 1)."""
    searched = ranges[..., 0] >= 0
    cx, cy, ax, ay = (lines[..., i] for i in range(4))
    out = dict(row_major=bool(((cx == 1.0) & (ax == 0.0))[searched].all()), horizontal=bool((cy[searched] == 0.0).all()),
               uniform=True, rows={}, open=[], outside=[])
    for y in range(ranges.shape[0]):
        v = ay[y][searched[y]]
        if v.size == 0:
            continue
        if (v != v[0]).any():
            out["uniform"] = False
        out["rows"][y] = float(v[0])
        lo, hi = float(v[0]) - CORRIDOR, float(v[0]) + CORRIDOR
        closed = lo > 8.0 and hi < 1.0e9 and np.frexp(lo)[1] == np.frexp(hi)[1]
        if not closed:
            out["open"].append(y)
        if np.floor(lo) < 1.0:
            out["outside"].append(y)
    return out
