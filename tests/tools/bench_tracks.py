"""Times the perspective tail of reconstruct_perspective with the dense track table on the host (resident_tracks=False, the
default) and in device memory (resident_tracks=True) in one process: config 5 at --size (default 2048^2, three
views), merge_tracks=True, bundle_adjustment=False, max_points = --max-points so that the subset stage runs; pairs_result is
computed once outside the timed region.  Per mode: the median (and min, max) over --repeat runs after one warm-up of the stages
dense, tracks, merge, triangulate and subset as ImageReconstruction._timed measures them (the device synchronised before and
after each), the sum tracks + merge + triangulate, and the bytes that crossed between host and device for the grid, the table
and the surface - counted from the arrays' sizes where the wrappers hand them to the library (scalar read-backs of a few bytes
per call, and the camera matrices, are not counted).  The two modes' tables and surfaces are compared once.
The match kernel's launches per pair are not counted here: run
`rocprofv3 --kernel-trace --stats -- python tests/tools/bench_tracks.py --size 512 --repeat 1 --mode host` (and `--mode
resident`) and read the extend_tracks_match_kernel row.

    python tests/tools/bench_tracks.py [--size 2048] [--repeat 5] [--max-points 1000000] [--mode both] [--out profiles/x.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from cybervision_amd import correlation, reconstruction, synth, triangulation  # noqa: E402

STAGES = ("dense", "tracks", "merge", "triangulate", "subset")


class Traffic:
    """Bytes between host and device, by the sizes of the arrays the wrappers pass: the methods are wrapped for the run."""

    def __init__(self):
        self.up = self.down = 0
        self.by_stage = {}
        self._saved = []

    def add(self, stage, up=0, down=0):
        self.up += up
        self.down += down
        s = self.by_stage.setdefault(stage, [0, 0])
        s[0] += up
        s[1] += down

    def _wrap(self, owner, name, make):
        old = getattr(owner, name)
        self._saved.append((owner, name, old))
        setattr(owner, name, make(old))

    def __enter__(self):
        tr = self

        def complete(old):
            def f(self, *a, out_xy=None, out_corr=None, **kw):
                if out_xy is None:  # host arrays: the whole grid comes down, (x, y) int32 and the f32 score per cell
                    tr.add("dense", down=self.w1 * self.h1 * 12)
                return old(self, *a, out_xy=out_xy, out_corr=out_corr, **kw)
            return f

        def extend_tracks(old):
            def f(self, track_p1, max_dimension2):
                out = old(self, track_p1, max_dimension2)
                n, new = len(out[0]), len(out[1])
                calls = 2 if new else 1  # (cap = 0 to size the buffers, then to fill them)
                tr.add("tracks", up=calls * n * 8, down=calls * n * 8 + new * 16)
                return out
            return f

        def merge_tracks(old):
            def f(self, device, image_index):
                out = old(self, device, image_index)
                if not self.resident_tracks:
                    tr.add("merge", up=out["rows_in"] * self.images_count * 8, down=out["rows_out"] * self.images_count * 8)
                return out
            return f

        def triangulate(old):
            def f(self, device, *a, **kw):
                n = len(self.tracks)
                s = old(self, device, *a, **kw)
                k, m = len(s.track_index), len(s.cameras)
                if self.resident_tracks:
                    tr.add("triangulate", down=k * 8)  # track_index
                else:
                    tr.add("triangulate", up=n * m * 8, down=k * (24 + 8))
                return s
            return f

        def subset(old):
            def f(device, surface, max_points, seed=0):
                out, info = old(device, surface, max_points, seed)
                n, k, m = info["rows_in"], info["rows_out"], len(surface.cameras)
                if hasattr(surface.points, "data_ptr"):
                    tr.add("subset", down=k * 8)  # the kept rows
                else:
                    tr.add("subset", up=n * (24 + m * 8), down=k * (8 + 24 + m * 8))
                return out, info
            return f

        self._wrap(correlation.PointCorrelations, "complete", complete)
        self._wrap(correlation.PointCorrelations, "extend_tracks", extend_tracks)
        self._wrap(triangulation.PerspectiveTriangulation, "merge_tracks", merge_tracks)
        self._wrap(triangulation.PerspectiveTriangulation, "triangulate_all_recovered", triangulate)
        self._wrap(triangulation, "subset", subset)
        return self

    def __exit__(self, *exc):
        for owner, name, old in reversed(self._saved):
            setattr(owner, name, old)
        self._saved = []


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--max-points", type=int, default=1_000_000)
    ap.add_argument("--mode", choices=("both", "host", "resident"), default="both")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    dev = correlation.create_gpu_context()
    views, K, _poses = synth.make_sfm_views(args.size)
    steps = synth.optimal_scale_steps(args.size, args.size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    pairs = reconstruction.reconstruct_pairs(dev, pyrs, dense=False, seed=3)
    result = {"size": args.size, "views": len(pyrs), "merge_tracks": True, "bundle_adjustment": False, "max_points": args.max_points,
              "repeat": args.repeat, "device": dev.name(), "modes": {}}
    last = {}
    for mode in ("host", "resident"):
        if args.mode not in ("both", mode):
            continue
        resident = mode == "resident"
        runs, traffic = [], None
        for it in range(args.repeat + 1):  # (the first run is the warm-up: code objects, the arena, the parked buffers)
            print(f"{mode} run {it}", file=sys.stderr, flush=True)
            with Traffic() as tr:
                out = reconstruction.reconstruct_perspective(dev, pyrs, K, bundle_adjustment=False, seed=3, pairs_result=pairs,
                                                             merge_tracks=True, max_points=args.max_points, max_points_seed=5,
                                                             resident_tracks=resident)
            if it:
                runs.append(out["timings_ms"])
            traffic = tr
            table = out["tracks"].numpy() if resident else out["tracks"]
            if resident:
                out["tracks"].close()
            last[mode] = (table, _host(out["surface"].points), out["surface"].track_index, _host(out["surface"].tracks))
            del out
        row = {"rows": int(len(last[mode][0])), "surface_rows": int(len(last[mode][1]))}
        for st in STAGES:
            t = [r.get(st, 0.0) for r in runs]
            row[st] = {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}
        tail = [r.get("tracks", 0.0) + r.get("merge", 0.0) + r.get("triangulate", 0.0) for r in runs]
        row["tracks_merge_triangulate"] = {"median_ms": round(statistics.median(tail), 3), "min_ms": round(min(tail), 3),
                                           "max_ms": round(max(tail), 3)}
        row["bytes_host_to_device"], row["bytes_device_to_host"] = int(traffic.up), int(traffic.down)
        row["bytes_by_stage"] = {k: {"up": int(v[0]), "down": int(v[1])} for k, v in traffic.by_stage.items()}
        result["modes"][mode] = row
    if len(last) == 2:
        result["same_results"] = bool(all(a.shape == b.shape and a.tobytes() == b.tobytes()
                                          for a, b in zip(last["host"], last["resident"])))
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    dev.close()


if __name__ == "__main__":
    main()
