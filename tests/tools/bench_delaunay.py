"""Times cvhip_mesh_delaunay on bench_mesh.py's surface: the size^2 jittered lattice, camera 0's points.
Reports the median and spread of the call with points and faces in device memory and in host memory, the statistics (the
host-star share, the largest cell count), a sweep of cvhip_mesh_delaunay_set_lane_cells (0 - every star on the host -
only with --with-host-only: it is minutes at 2048^2) and, when scipy is importable, mesh.delaunay_scipy's time on the same
points on the same machine - the only way to do this step before cvhip_mesh_delaunay.

    python tests/tools/bench_delaunay.py [--size 2048] [--repeat 5] [--sweep 128,256,...] [--out profiles/x.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import bench_mesh  # noqa: E402
from cybervision_amd import _lib, correlation, mesh  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sweep", default="128,256,512,1024,2048,4096,16384,4294967295")
    ap.add_argument("--with-host-only", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    X, tracks, P, r, t, dims, _, _ = bench_mesh.build_surface(args.size)
    dev = correlation.create_gpu_context()
    L = _lib.lib()
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    dp = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    surf = [hp(X), hp(tracks), len(X), 3, hp(P), hp(r), hp(t), hp(dims)]
    cnt = C.c_uint64(0)
    _lib.check(L.cvhip_mesh_camera_points(dev.handle, *surf, 0, None, None, 0, C.byref(cnt)), "camera_points")
    k = cnt.value
    idx, xy = np.zeros(k, dtype=np.uint32), np.zeros((k, 2))
    _lib.check(L.cvhip_mesh_camera_points(dev.handle, *surf, 0, hp(idx), hp(xy), k, C.byref(cnt)), "camera_points")
    d_xy = torch.from_numpy(xy).cuda()
    d_faces = torch.zeros((2 * k, 3), dtype=torch.int32, device="cuda")
    h_faces = np.zeros((2 * k, 3), dtype=np.uint32)
    torch.cuda.synchronize()
    n, st = C.c_uint64(0), np.zeros(len(mesh.DELAUNAY_STATS), dtype=np.uint64)

    def device_call():
        _lib.check(L.cvhip_mesh_delaunay(dev.handle, dp(d_xy), k, dp(d_faces), 2 * k, C.byref(n), hp(st)), "delaunay")

    def host_call():
        _lib.check(L.cvhip_mesh_delaunay(dev.handle, hp(xy), k, hp(h_faces), 2 * k, C.byref(n), hp(st)), "delaunay")

    def timed(fn, repeat):
        print(f"timing {getattr(fn, '__name__', 'call')} x {repeat}", file=sys.stderr, flush=True)
        times = []
        for _ in range(repeat):
            t1 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t1) * 1e3)
        return {"median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3),
                "runs": repeat}

    result = {"size": args.size, "points": k, "device": dev.name() if hasattr(dev, "name") else "",
              "lane_cells_default": mesh.DELAUNAY_LANE_CELLS_DEFAULT}
    device_call()  # (warm-up: the first launch loads the code object)
    result["device_memory"] = timed(device_call, args.repeat)
    result["faces"] = n.value
    result["stats"] = dict(zip(mesh.DELAUNAY_STATS, (int(v) for v in st)))
    result["host_star_share"] = result["stats"]["host_stars"] / max(k, 1)
    result["host_memory"] = timed(host_call, args.repeat)
    first = d_faces[:n.value].clone()
    sweep = [int(v) for v in args.sweep.split(",")] + ([0] if args.with_host_only else [])
    result["sweep"] = []
    for cells in sweep:
        mesh.set_delaunay_lane_cells(dev, cells)
        print(f"lane_cells {cells}", file=sys.stderr, flush=True)
        row = {"lane_cells": cells, **timed(device_call, 1 if cells == 0 else max(2, args.repeat // 2))}
        row["host_stars"], row["most_cells"] = int(st[3]), int(st[5])
        row["same_faces"] = bool(n.value == len(first) and torch.equal(d_faces[:n.value], first))
        result["sweep"].append(row)
    mesh.set_delaunay_lane_cells(dev, mesh.DELAUNAY_LANE_CELLS_DEFAULT)
    if not args.no_scipy:
        try:
            import scipy  # noqa: F401

            result["delaunay_scipy"] = timed(lambda: mesh.delaunay_scipy(xy), 1)
        except ImportError:
            result["delaunay_scipy"] = None
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
