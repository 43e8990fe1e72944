#!/usr/bin/env python3
"""Perspective triangulation on config 5's scene (three 2048^2 views, synth.make_sfm_views) with the true cameras: the
sparse stage and the dense pair loop build the track table (reconstruct_perspective_surface), then
cvhip_triangulate_perspective runs on that table without and with bundle adjustment.  Prints ONE JSON line: track and kept
counts, ms for triangulate + filter, ms per bundle-adjustment iteration (the difference of the two calls over the
iterations), the iteration count and the total, and the CPU restatement (tests/ref_triangulation.py, numpy) on a stated
subset of the tracks with the host's core count.   usage: triangulation_bench.py [size] [repeats]"""
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402

from cybervision_amd import correlation, reconstruction, synth, triangulation  # noqa: E402

SIZE = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
SUBSET = 20_000

dev = correlation.create_gpu_context()
views, K, poses = synth.make_sfm_views(SIZE)
steps = synth.optimal_scale_steps(SIZE, SIZE)
pyrs = [synth.box_pyramid(v, steps) for v in views]
cams = [(K, R, t) for R, t in poses]
pairs = reconstruction.reconstruct_pairs(dev, pyrs, dense=False)
out = reconstruction.reconstruct_perspective_surface(dev, pyrs, pairs, cams, bundle_adjustment=False)
table = out["tracks"]


def timed(ba):
    tri = triangulation.PerspectiveTriangulation(3, [(SIZE, SIZE)] * 3, bundle_adjustment=ba)
    tri.tracks = table
    best, surf = None, None
    for _ in range(REPEATS):
        dev.synchronize()
        t0 = time.perf_counter()
        surf = tri.triangulate_all(dev, cams)
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best, surf


ms_off, surf_off = timed(False)
ms_on, surf_on = timed(True)
iters = surf_on.ba_iterations
ms_iter = (ms_on - ms_off) / iters if iters else None

import ref_triangulation as rt  # noqa: E402

sub = table[:SUBSET]
t0 = time.perf_counter()
idx, pts, _, ba = rt.triangulate_all(sub, cams, bundle_adjustment=False)
cpu_tri_ms = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
idx, pts, _, ba = rt.triangulate_all(sub, cams, bundle_adjustment=True)
cpu_ba_ms = (time.perf_counter() - t0) * 1e3 - cpu_tri_ms

n_obs = int((surf_on.tracks[..., 0] >= 0).sum())
print(json.dumps({
    "scene": f"config 5 (synth.make_sfm_views {SIZE}^2, 3 views, true cameras)",
    "tracks": int(len(table)), "kept": int(len(surf_on.points)),
    "dense_and_tracks_ms": {k: round(v, 2) for k, v in out["timings_ms"].items() if k in ("dense", "tracks")},
    "triangulate_filter_ms": round(ms_off, 3),
    "ba_iterations": iters, "ba_history": surf_on.ba_history,
    "ba_ms_per_iteration": None if ms_iter is None else round(ms_iter, 3),
    "ba_total_ms": round(ms_on - ms_off, 3), "triangulate_all_ms": round(ms_on, 3),
    "reprojection_rms_px": [round(v / np.sqrt(n_obs), 5) for v in surf_on.ba_residual_norms],
    "cpu_restatement": {"subset_tracks": SUBSET, "cores": os.cpu_count(), "triangulate_filter_ms": round(cpu_tri_ms, 1),
                        "ba_ms": round(cpu_ba_ms, 1), "ba_iterations": len(ba.history),
                        "note": "numpy restatement (tests/ref_triangulation.py) on the first tracks of the table - a subset"},
}))
