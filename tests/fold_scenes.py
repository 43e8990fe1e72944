"""The lean box walk's fold (box_body.inc) restated in plain Python, and the scenes that exercise it.

A wave of the lean box kernel walks the union of its lanes' displacement intervals, n steps.  Where the intervals drift
along the wave, the first steps are searched only at one end of it and the last steps only at the other; low step k and
high step n - K + k (k = 0 .. K-1) then run as one step, the lanes on one side of a seam at the low step and the lanes on
the other side at the high one.  A lane's window sum is P(l) - P(l - 11), the sum of the column products of lanes
l-10 .. l, so a lane's result is right exactly when those eleven lanes share its step.

`schedule` is the rule as stated (envelopes over the steps, the largest K by trial), `schedule_closed` what the kernel
computes (two prefix scans over the lanes, two wave minima, no table over the steps), `lane_steps` the walk that follows
from it and `check_walk` the brute-force proof obligations.  The scenes are rectified pairs with a chosen integer
disparity field; `lane_waves` regroups the oracle's last-level ranges into the kernel's waves, lane by lane."""
from __future__ import annotations

import numpy as np

import box_scenes
from cybervision_amd import synth

LANES = 64
LANE0 = 11    # lanes 0..10 carry the halo columns of lane 11's window and search nothing
WINDOW = 11   # a lane's window: the columns of lanes l-10 .. l
S3_OUT = box_scenes.S3_OUT
KERNEL_SIZE = box_scenes.KERNEL_SIZE
MAX_STEPS = 65
BIG = 1 << 30


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def schedule(lo, hi, has):
    """The rule as the design states it.  lo, hi: per-lane interval in steps (inclusive), has: lane searches at all.
    n = the union's length.  -> (K, descending, seams): seams[k] = the last lane of the LOWER side of pair k."""
    lanes = [l for l in range(LANES) if has[l]]
    if not lanes:
        return 0, False, []
    n = max(hi[l] for l in lanes) + 1
    best = (0, False, [])
    for desc in (False, True):
        for K in range(n // 2, 0, -1):
            seams = []
            for k in range(K):
                t = n - K + k
                # supersets of the lanes that search steps k and t (neither is empty: some interval starts at step 0 and
                # some interval ends at step n - 1)
                low = [l for l in lanes if lo[l] <= k]
                high = [l for l in lanes if hi[l] >= t]
                if not desc:
                    # ascending: low steps live at low lanes
                    maxlane_lo = max(low)
                    minlane_hi = min(high)
                    if not maxlane_lo + 10 < minlane_hi:
                        break
                    seams.append(maxlane_lo)
                else:
                    minlane_lo = min(low)
                    maxlane_hi = max(high)
                    if not maxlane_hi + 10 < minlane_lo:
                        break
                    seams.append(maxlane_hi)
            else:
                if K > best[0]:
                    best = (K, desc, seams)
                break
    return best


def schedule_closed(lo, hi, has):
    """What the kernel computes.  -> (K, descending, sel [per lane], base): at folded pair k a lane takes the high step
    n - K + k iff sel[lane] >= base + k, else the low step k."""
    lanes = [l for l in range(LANES) if has[l]]
    if not lanes:
        return 0, False, [0] * LANES, 0
    n = max(hi[l] for l in lanes) + 1
    hpre, lpre, h, m = [], [], -1, BIG
    for l in range(LANES):  # inclusive prefix maximum of hi / minimum of lo over the lanes
        if has[l]:
            h, m = max(h, hi[l]), min(m, lo[l])
        hpre.append(h)
        lpre.append(m)
    mh = [hpre[min(l + 10, LANES - 1)] for l in range(LANES)]
    ml = [lpre[min(l + 10, LANES - 1)] for l in range(LANES)]
    ka = min(min(n + lo[l] - mh[l] for l in lanes) - 1, n // 2)
    kd = min(min(n + ml[l] - hi[l] for l in lanes) - 1, n // 2)
    if kd > ka:
        return kd, True, ml, 1
    return ka, False, mh, n - ka


def lane_steps(n, K, sel, base, fold=True):
    """The walk: a list of rounds, each the per-lane step.  The steps [K, n - K) nobody folded run first, inside out
    from their middle; the folded pairs follow, pair K-1 first."""
    if not fold:
        K = 0
    nmid = n - 2 * K
    mid = nmid >> 1
    rounds = []
    for t in range(nmid):
        s = K + (mid + t if t < nmid - mid else nmid - 1 - t)
        rounds.append([s] * LANES)
    for k in range(K - 1, -1, -1):
        rounds.append([n - K + k if sel[l] >= base + k else k for l in range(LANES)])
    return rounds


def plain_walk(n):
    """The walk before the fold existed: every step of the union, inside out."""
    mid = n >> 1
    return [[mid + t if t < n - mid else n - 1 - t] * LANES for t in range(n)]


def check_walk(lo, hi, has, rounds):
    """Every (lane, step of its own interval) is visited exactly once, and at each visit lanes l-10 .. l share the
    lane's step.  -> number of visits."""
    seen = {}
    for r in rounds:
        for l in range(LANES):
            if has[l] and lo[l] <= r[l] <= hi[l]:
                assert (l, r[l]) not in seen, f"lane {l} visits step {r[l]} twice"
                seen[(l, r[l])] = True
                assert all(r[j] == r[l] for j in range(l - WINDOW + 1, l + 1)), f"lane {l}: its window is split at step {r[l]}"
    want = sum(hi[l] - lo[l] + 1 for l in range(LANES) if has[l])
    assert len(seen) == want, f"{want - len(seen)} (lane, step) pairs are never visited"
    return want


# ---------------------------------------------------------------------------------------------------------------------
# random waves
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = ("rising", "falling", "tent", "valley", "edge", "noise")


def random_wave(rng, shape):
    """-> (lo, hi, has) of one wave: interval centres of the given shape along the lanes, lengths that vary a little,
    some lanes without a pixel, the union shifted to start at step 0 and clipped to MAX_STEPS."""
    l = np.arange(LANES)
    amp = rng.integers(0, 56)
    apex = rng.integers(LANE0, LANES)
    if shape == "rising":
        c = amp * (l - LANE0) / (LANES - LANE0)
    elif shape == "falling":
        c = amp * (LANES - 1 - l) / (LANES - LANE0)
    elif shape == "tent":
        c = amp - amp * np.abs(l - apex) / (LANES - LANE0)
    elif shape == "valley":
        c = amp * np.abs(l - apex) / (LANES - LANE0)
    elif shape == "edge":
        c = np.where(l >= apex, amp, 0) * (1 if rng.integers(0, 2) else -1)
    else:
        c = rng.integers(0, amp + 1, LANES)
    half = rng.integers(0, 12) + rng.integers(0, 3, LANES)
    lo = np.floor(c - half).astype(np.int64)
    hi = np.floor(c + half).astype(np.int64) + rng.integers(0, 2, LANES)
    has = l >= LANE0
    mode = rng.integers(0, 4)
    if mode == 1:
        has &= rng.random(LANES) > 0.2
    elif mode == 2:  # a run of lanes without pixels inside the wave, or the wave's end missing (the image's edge)
        a = rng.integers(LANE0, LANES)
        has &= ~((l >= a) & (l < a + rng.integers(1, 30)))
    if not has.any():
        has[rng.integers(LANE0, LANES)] = True
    base = lo[has].min()
    lo, hi = lo - base, hi - base
    # n from 1 to MAX_STEPS: the union cut at the kernel's limit, every other time at a random step below it
    top = min(int(hi[has].max()), MAX_STEPS - 1 if rng.integers(0, 2) else rng.integers(0, MAX_STEPS))
    hi = np.minimum(hi, top)
    lo = np.minimum(lo, hi)
    lo[has] -= lo[has].min()
    return [int(v) for v in lo], [int(v) for v in hi], [bool(v) for v in has]


# ---------------------------------------------------------------------------------------------------------------------
# scenes: rectified pairs with a chosen disparity field
# ---------------------------------------------------------------------------------------------------------------------
def _ramp(w, h, num, den):
    x = np.arange(w, dtype=np.int64)[None, :]
    return np.broadcast_to((x * num) // den, (h, w)).copy()


def _field(name, w, h):
    x = np.arange(w, dtype=np.int64)[None, :]
    if name == "ramp_up":
        d = (x * 1) // 4
    elif name == "ramp_down":
        d = -((x * 1) // 4)
    elif name == "flat":
        d = 0 * x
    elif name == "tent_valley":  # apexes every 90 columns: inside waves (53 pixels), never at the same lane twice
        u = np.mod(x, 180)
        d = np.where(u < 90, u, 180 - u) // 4
    elif name == "edge":         # 12 px at columns that are no multiple of 53
        d = np.where((x >= 131) & (x < 297), 12, 0)
    elif name == "ramp_half":
        d = (x * 7) // 16
    elif name == "ramp_strip":
        d = (x * 1) // 4
    else:
        raise KeyError(name)
    return np.broadcast_to(d, (h, w)).copy()


# name -> (width, height, texture seed)
SCENES = {
    "ramp_up": (424, 128, 31),
    "ramp_down": (424, 128, 32),
    "flat": (424, 128, 33),
    "tent_valley": (512, 128, 34),
    "edge": (424, 128, 35),
    "ramp_half": (318, 128, 36),
    "ramp_strip": (53 * 7 + 7, 128, 37),
}


def make_scene(name):
    """name -> dict(name, img1, img2, F, projection, steps), as cases.make_case.  img1 = T(x, y), img2(x, y) =
    T(x + d(x, y), y) as synth.make_pair makes them, for the scene's own integer disparity field.  Deterministic."""
    w, h, seed = SCENES[name]
    d = _field(name, w, h)
    # image 2 is wider by the largest displacement, so that displaced pixels stay inside it (its texture continues there)
    a, b = box_scenes.stepped_pair(w, h, d, 0.0, seed, pad=int(np.abs(d).max()) + 8 if d.any() else 0)
    b = b[:h]
    if name == "ramp_strip":
        # a strip without texture: its pixels' windows have no deviation, are skipped by the reference (min_stdev) and
        # leave lanes without a pixel inside waves
        a = a.copy()
        a[:, 150:190] = 90
        a[20:40, 60:300] = 90
    c = dict(name=name, img1=np.ascontiguousarray(a), img2=np.ascontiguousarray(b),
             F=np.asarray(synth.F_HORIZONTAL, dtype=np.float64), projection=0,
             steps=synth.optimal_scale_steps(a.shape[1], a.shape[0]))
    if name == "flat":
        # Two identical images.  A pixel's range is centred on the mean POSITION of the previous level's matches around it
        # (estimate_search_range), so next to the border of what was matched the ranges drift whatever the disparity does.
        # This scene keeps that out of the last level: its full-resolution images lose their texture within FLAT_BORDER
        # columns of the left and right border - nothing is searched there (min_stdev) - while the coarser levels come
        # from the untouched images and match everywhere.
        p1, p2 = synth.box_pyramid(c["img1"], c["steps"]), synth.box_pyramid(c["img2"], c["steps"])
        for p in (p1, p2):
            p[0] = p[0].copy()
            p[0][:, :FLAT_BORDER] = 90
            p[0][:, p[0].shape[1] - FLAT_BORDER:] = 90
        c["img1"], c["img2"], c["pyramids"] = p1[0], p2[0], (p1, p2)
    return c


FLAT_BORDER = 32


def pyramids(c):
    """The level images the scene is run on, coarse levels last (cases.pyramids, unless the scene brings its own)."""
    if "pyramids" in c:
        return c["pyramids"]
    return synth.box_pyramid(c["img1"], c["steps"]), synth.box_pyramid(c["img2"], c["steps"])


def last_ranges(oracle, c):
    """box_scenes.oracle_last_ranges over the scene's own level images."""
    if "pyramids" not in c:
        return box_scenes.oracle_last_ranges(oracle, c)
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


def lane_waves(ranges, lines, dims2):
    """The lean box kernel's waves over one direction's last-level ranges, lane by lane (box_body.inc: setup and box
    reduction; row-major tiles, lines along x).  -> list of dict(v, u0, n, lo, hi, has), lo / hi in steps from the
    wave's first displacement.  The unions agree with box_scenes.box_waves."""
    h, w = ranges.shape[:2]
    w2, _ = dims2
    r0, r1 = ranges[..., 0].astype(np.int64), ranges[..., 1].astype(np.int64)
    ilo = np.maximum(r0, KERNEL_SIZE)
    ihi = np.minimum(r1, max(w2 - KERNEL_SIZE, 0))
    own = (r0 >= 0) & (ihi > ilo)
    out = []
    for v in range(h):
        for u0 in range(0, w, S3_OUT):
            lo, hi, has = [0] * LANES, [0] * LANES, [False] * LANES
            for l in range(LANE0, LANES):
                x = u0 + l - LANE0
                if x < w and own[v, x]:
                    has[l] = True
                    lo[l], hi[l] = int(ilo[v, x]) - x, int(ihi[v, x]) - 1 - x
            if not any(has):
                continue
            mn = min(lo[l] for l in range(LANES) if has[l])
            mx = max(hi[l] for l in range(LANES) if has[l])
            out.append(dict(v=v, u0=u0, n=mx - mn + 1, mn=mn, mx=mx, has=has,
                            lo=[lo[l] - mn if has[l] else 0 for l in range(LANES)],
                            hi=[hi[l] - mn if has[l] else 0 for l in range(LANES)]))
    return out


WG_ROWS = box_scenes.WG_ROWS
S3_COLS = 128  # target columns a workgroup stages per copy (lean plan)
PLANES = 5     # a rectified pixel's stripes (corridor_size 2): the planes of a lean workgroup


def admitted(waves):
    """The waves whose workgroup the lean plan admits (box_body.inc, `eligible`): the workgroup's displacement box - the
    union over its four rows - fits the staged columns at its alignment, and is no more than three times (and 16) the
    largest candidate set of one of its pixels.  The other workgroups decline as a whole and walk nothing."""
    wg = {}
    for wv in waves:
        longest = max(wv["hi"][l] - wv["lo"][l] + 1 for l in range(LANES) if wv["has"][l])
        k = (wv["v"] // WG_ROWS, wv["u0"])
        lo, hi, ln = wg.get(k, (wv["mn"], wv["mx"], 0))
        wg[k] = (min(lo, wv["mn"]), max(hi, wv["mx"]), max(ln, longest))
    out = []
    for wv in waves:
        lo, hi, ln = wg[(wv["v"] // WG_ROWS, wv["u0"])]
        W, colshift = hi - lo + 1, (wv["u0"] - 6 + lo) & 3
        if colshift + 64 + W - 1 <= S3_COLS and W * PLANES <= 3 * ln * PLANES + 16:
            out.append(wv)
    return out


def scene_folds(oracle, c, only_admitted=False):
    """-> dict(union, folded, asc, desc, waves_asc, waves_desc, waves, declined): the fold of every lean wave of the
    scene's last level, both directions, from the oracle's ranges; only_admitted: of the waves whose workgroup the lean
    plan admits - what the kernel's counters report."""
    tot = dict(union=0, folded=0, asc=0, desc=0, waves_asc=0, waves_desc=0, waves=0, declined=0)
    for direction, (r, lines) in enumerate(last_ranges(oracle, c)):
        h2, w2 = (c["img2"] if direction == 0 else c["img1"]).shape
        waves = lane_waves(r, lines, (w2, h2))
        if only_admitted:
            tot["declined"] += len(waves) - len(admitted(waves))
            waves = admitted(waves)
        for wv in waves:
            K, desc, _, _ = schedule_closed(wv["lo"], wv["hi"], wv["has"])
            tot["waves"] += 1
            tot["union"] += wv["n"]
            tot["folded"] += wv["n"] - K
            tot["desc" if desc else "asc"] += K
            if K:
                tot["waves_desc" if desc else "waves_asc"] += 1
    return tot
