"""Scenes for the stepped box walk (box_body.inc): pairs whose search ranges at the last level give waves of the box
kernel a displacement range of exactly 65 steps along a sloped epipolar line - one more than the 64 lanes of the
walk's step table - and a restatement of the kernel's wave grouping that shows it from the oracle's ranges alone.

A disparity field that jumps between two values makes the neighbours of a pixel near the jump disagree: the previous
level's matches around it spread, estimate_search_range (oracle/cvref_corr.c) turns that spread into a long interval,
and the interval's centre moves with the mix.  Along one wave's 53 pixels the intervals then cover more displacements
than any single one of them."""
from __future__ import annotations

import math

import numpy as np

from cybervision_amd import synth

KERNEL_SIZE = 5
S3_OUT = 53   # searched pixels per wave (lanes 11..63)
WG_ROWS = 4   # waves per workgroup: consecutive rows (columns for transposed tiles)
TABLE = 64    # steps of the walk's per-wave step table (one per lane)


def stepped_pair(width, height, d, tilt_deg, seed, pad=0):
    """img1 = T(x, y), img2(x, y) = T(x + d cos, y + d sin) as in synth.make_pair, for a given integer disparity field
    d [height, width]; img2 gets `pad` more columns and rows (its texture continues there with d = 0)."""
    xs = np.arange(width + pad, dtype=np.int64)[None, :]
    ys = np.arange(height + pad, dtype=np.int64)[:, None]
    dd = np.zeros((height + pad, width + pad), dtype=np.int64)
    dd[:height, :width] = d
    ci = int(round(math.cos(math.radians(tilt_deg)) * 65536.0))
    si = int(round(math.sin(math.radians(tilt_deg)) * 65536.0))
    t1 = synth.texture(xs[:, :width], ys[:height], seed)
    t2 = synth.texture(xs + ((dd * ci + 32768) >> 16), ys + ((dd * si + 32768) >> 16), seed)
    return (np.ascontiguousarray(np.clip(t1, 0, 255).astype(np.uint8)),
            np.ascontiguousarray(np.clip(t2, 0, 255).astype(np.uint8)))


def step_field(width, height, period, jump, axis=1):
    """0 / jump in alternate bands of period / 2 pixels along `axis` (1: bands of columns, 0: of rows)."""
    v = np.arange(width if axis == 1 else height, dtype=np.int64)
    band = np.where((v % period) >= period // 2, jump, 0)
    return np.broadcast_to(band[None, :] if axis == 1 else band[:, None], (height, width)).copy()


def oracle_last_ranges(oracle, c):
    """Run the oracle's level loop over the case's pyramids and return, per direction, the last level's search
    ranges [h, w, 2] (-1 where the pixel is not searched) and epipolar lines [h, w, 4]."""
    p1, p2 = synth.box_pyramid(c["img1"], c["steps"]), synth.box_pyramid(c["img2"], c["steps"])
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


def box_waves(ranges, lines, dims2, corridor_size):
    """The box kernel's waves over one direction's last-level ranges (box_body.inc, setup and box reduction).

    Tiles are row-major (a wave = 53 pixels of one row, lines along x) or transposed (53 pixels of one column,
    lines along y) as the pixels' lines run.  For every wave with a searched pixel: the tile kind, its workgroup,
    the union [mn, mx] of its pixels' displacement intervals along the lines, the workgroup's union, the longest
    interval of any of its pixels, and whether some pixel's line changes row between the wave's first and last step.
    -> list of dicts."""
    h, w = ranges.shape[:2]
    w2, h2 = dims2
    r0, r1 = ranges[..., 0].astype(np.int64), ranges[..., 1].astype(np.int64)
    searched = r0 >= 0
    along_x = ~((lines[..., 1] == 1.0) & (np.abs(lines[..., 0]) < 1.0))  # coeff_x == 1: candidates advance along x
    out = []
    for tr in (False, True):
        lim2 = h2 if tr else w2
        ilo = np.maximum(r0, KERNEL_SIZE)
        ihi = np.minimum(r1, max(lim2 - KERNEL_SIZE, 0))
        own = searched & (along_x != tr) & (ihi > ilo)
        rows, cols = (w, h) if tr else (h, w)  # waves along `cols`, WG_ROWS of them per workgroup
        for v in range(rows):
            for u0 in range(0, cols, S3_OUT):
                u = np.arange(u0, min(u0 + S3_OUT, cols))
                ys, xs = (u, np.full_like(u, v)) if tr else (np.full_like(u, v), u)
                m = own[ys, xs]
                if not m.any():
                    continue
                pos = ys if tr else xs
                lo = ilo[ys, xs][m] - pos[m]
                hi = ihi[ys, xs][m] - 1 - pos[m]
                mn, mx = int(lo.min()), int(hi.max())
                # the lines' minor coordinate (floor of stripe -cs) at the wave's first and last step
                ln = lines[ys, xs][m]
                maj = pos[m]
                c, a = (ln[:, 0], ln[:, 2]) if tr else (ln[:, 1], ln[:, 3])
                first = np.floor(c * (maj + mn) + a - corridor_size)
                last = np.floor(c * (maj + mx) + a - corridor_size)
                out.append(dict(tr=tr, v=v, u0=u0, wg=(v // WG_ROWS, u0 // S3_OUT), mn=mn, mx=mx, steps=mx - mn + 1,
                                longest=int((ihi[ys, xs][m] - ilo[ys, xs][m]).max()),
                                steps_row=bool((first != last).any())))
    wg = {}
    for wv in out:
        k = (wv["tr"], wv["wg"])
        lo, hi, ln = wg.get(k, (wv["mn"], wv["mx"], 0))
        wg[k] = (min(lo, wv["mn"]), max(hi, wv["mx"]), max(ln, wv["longest"]))
    for wv in out:
        lo, hi, ln = wg[(wv["tr"], wv["wg"])]
        wv["wg_steps"] = hi - lo + 1
        wv["wg_longest"] = ln
        # the byte alignment of the workgroup's first staged target column (row-major tiles stage 4-column groups): the
        # wide plan holds 128 - 64 + 1 - colshift steps
        wv["colshift"] = 0 if wv["tr"] else (wv["u0"] - 6 + lo) & 3
    return out


def table_overruns(waves):
    """The waves that walk one step past the table: 65 steps, in a workgroup that the wide plan's box width and the
    per-pixel limit (64 candidates along the line) admit, with a line that changes row over them."""
    return [wv for wv in waves if wv["steps"] == TABLE + 1 and wv["wg_steps"] == TABLE + 1 and wv["colshift"] == 0
            and wv["wg_longest"] <= TABLE and wv["steps_row"]]


# name -> (width, height, band period, jump, tilt of the lines in degrees, texture seed, transposed).  img2 is padded by
# 64 pixels on both axes so that the displaced bands stay inside it.  Row-major: lines 2 degrees off the x axis, the
# wide stepped plan's tiles (about one row-major tile in four starts at a 4-column boundary: colshift 0).  Transposed:
# the same pair transposed, lines 2 degrees off the y axis (f_tilt(88)).
# No projection-1 scene (nine stripes): its intervals are 0.75 + 0.5 stdev long on either side of the centre, half the
# affine parameters' slope, so a pixel needs twice the neighbour spread for the same interval.  Bands of 64 pixels with
# jumps of 60..100 gave no 65-step wave in a workgroup the wide plan admits: the mixed pixels' intervals went past 64
# candidates (the whole workgroup then declines) before any wave's union reached 65 steps.
SCENES = {
    "bands_rows_256x160": (256, 160, 128, 32, 2.0, 5, False),
    "bands_cols_160x256": (256, 160, 128, 32, 2.0, 5, True),
}


def make_scene(name):
    """name -> dict(name, img1, img2, F, projection, steps, transposed), as cases.make_case.  Deterministic."""
    w, h, period, jump, tilt, seed, transposed = SCENES[name]
    a, b = stepped_pair(w, h, step_field(w, h, period, jump), tilt, seed, pad=64)
    F = synth.f_tilt(tilt)
    if transposed:
        a, b = np.ascontiguousarray(a.T), np.ascontiguousarray(b.T)
        F = synth.f_tilt(90.0 - tilt)
    return dict(name=name, img1=a, img2=b, F=np.asarray(F, dtype=np.float64), projection=0,
                steps=synth.optimal_scale_steps(a.shape[1], a.shape[0]), transposed=transposed)
