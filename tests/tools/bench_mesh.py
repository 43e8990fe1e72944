"""Times the mesh stage (cvhip_mesh_*) on a synthetic three-camera surface: a jittered lattice of size^2
tracks on a gently rolling surface, two triangles per lattice cell (the lattice split stands in for the Delaunay), and a
few long triangles that span most of a buffer (the hull slivers of a real triangulation).  Points, tracks and polygons are
resident on the device; every entry point synchronises, so wall time around a call is its time.  Reports, per stage, the
best of --repeat runs, the narrow / wide polygon counts, and a sweep of cvhip_mesh_set_wide_threshold.

    python tests/tools/bench_mesh.py [--size 2048] [--repeat 3] [--thresholds 0,64,...] [--out profiles/x.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from cybervision_amd import _lib, correlation, mesh  # noqa: E402


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def build_surface(size, seed=1):
    """-> (points [n, 3], tracks [n, 3, 2], P [3, 12], r [3, 3], t [3, 3], dims [3, 2], polygons [p, 3], long count)."""
    rng = np.random.default_rng(seed)
    f = float(size)
    K = np.array([[f, 0.0, size / 2.0], [0.0, f, size / 2.0], [0.0, 0.0, 1.0]])
    gy, gx = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing="ij")
    px = gx + rng.uniform(0.2, 0.8, gx.shape)
    py = gy + rng.uniform(0.2, 0.8, gy.shape)
    Z = 5.0 + 0.15 * np.sin(px * (6.0 / size)) * np.cos(py * (5.0 / size)) + rng.uniform(-1e-3, 1e-3, gx.shape)
    X = np.stack([(px - size / 2.0) / f * Z, (py - size / 2.0) / f * Z, Z], axis=-1).reshape(-1, 3)
    thetas = [0.0, math.radians(8.0), math.radians(-10.0)]
    P, r, t = [], [], []
    tracks = np.full((len(X), 3, 2), -1, dtype=np.int32)
    for j, th in enumerate(thetas):
        Cc = np.array([5.0 * math.sin(th), 0.0, 5.0 - 5.0 * math.cos(th)])
        R = rot_y(th)
        tj = -R @ Cc
        P.append((K @ np.hstack([R, tj[:, None]])).reshape(12))
        r.append(np.array([0.0, th, 0.0]))  # matrix_r((0, th, 0)) = rot_y(th)
        t.append(tj)
        q = (X @ R.T + tj) @ K.T
        p = np.round(q[:, :2] / q[:, 2:3])
        ok = (p >= 0).all(axis=1) & (p < size).all(axis=1) & (rng.random(len(X)) < 0.9)
        tracks[ok, j] = p[ok].astype(np.int32)
    rr, cc = np.meshgrid(np.arange(size - 1), np.arange(size - 1), indexing="ij")
    v00 = (rr * size + cc).ravel()
    lattice = np.concatenate([np.stack([v00, v00 + 1, v00 + size + 1], axis=1), np.stack([v00, v00 + size + 1, v00 + size], axis=1)])
    n = len(X)
    far = rng.integers(0, n, size=(64, 3))  # long triangles between random far-apart points
    polygons = np.concatenate([lattice, far]).astype(np.uint32)
    dims = np.full((3, 2), size, dtype=np.uint32)
    return X, tracks, np.stack(P), np.stack(r), np.stack(t), dims, polygons, len(far)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--thresholds", default="0,16,64,256,1024,2048,4096,16384,65536,4294967295")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    t0 = time.perf_counter()
    X, tracks, P, r, t, dims, polygons, n_long = build_surface(args.size)
    build_s = time.perf_counter() - t0
    n, n_poly, m = len(X), len(polygons), 3
    dev = correlation.create_gpu_context()
    L = _lib.lib()
    d_pts, d_tracks = torch.from_numpy(X).cuda(), torch.from_numpy(tracks).cuda()
    d_poly = torch.from_numpy(polygons.view(np.int32)).cuda()
    d_keep = torch.zeros(n_poly, dtype=torch.uint8, device="cuda")
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    dp = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    surf = [dp(d_pts), dp(d_tracks), n, m, hp(P), hp(r), hp(t), hp(dims)]
    torch.cuda.synchronize()  # (torch fills on its own stream, the library works on the handle's)

    def best(fn):
        times = []
        for _ in range(args.repeat):
            t1 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t1) * 1e3)
        return min(times)

    result = {"size": args.size, "tracks": n, "polygons": n_poly, "long_polygons": n_long, "cameras": m, "device": dev.name()
              if hasattr(dev, "name") else "", "build_scene_s": round(build_s, 2), "stages_ms": {}, "sweep": []}
    cnt = C.c_uint64(0)
    result["stages_ms"]["camera_points_count"] = best(lambda: _lib.check(L.cvhip_mesh_camera_points(
        dev.handle, *surf, 0, None, None, 0, C.byref(cnt)), "camera_points"))
    k = cnt.value
    d_idx = torch.zeros(k, dtype=torch.int32, device="cuda")
    d_xy = torch.zeros((k, 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    result["stages_ms"]["camera_points"] = best(lambda: _lib.check(L.cvhip_mesh_camera_points(
        dev.handle, *surf, 0, dp(d_idx), dp(d_xy), k, C.byref(cnt)), "camera_points"))
    result["camera_points_0"] = k
    w, h = C.c_uint64(0), C.c_uint64(0)
    result["stages_ms"]["depth_buffer_size_only"] = best(lambda: _lib.check(L.cvhip_mesh_depth_buffer(
        dev.handle, *surf, 1, None, 0, C.byref(w), C.byref(h)), "depth_buffer"))
    d_buf = torch.zeros(w.value * h.value, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    result["stages_ms"]["depth_buffer"] = best(lambda: _lib.check(L.cvhip_mesh_depth_buffer(
        dev.handle, *surf, 1, dp(d_buf), d_buf.numel(), C.byref(w), C.byref(h)), "depth_buffer"))
    result["buffer_1"] = [w.value, h.value]
    stats = np.zeros((m, 5), dtype=np.uint64)
    origin, minmax, wide = np.zeros(2), np.zeros(2), C.c_uint64(0)
    _lib.check(L.cvhip_mesh_depth_image(dev.handle, *surf, 0, -1.0, dp(d_poly), n_poly, None, 0, C.byref(w), C.byref(h), hp(origin),
                                        None, None), "depth_image")
    d_map = torch.zeros(w.value * h.value, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    result["image"] = [w.value, h.value]
    first_keep = None
    for thr in [int(v) for v in args.thresholds.split(",")]:
        mesh.set_wide_threshold(dev, thr)
        cull_ms = best(lambda: _lib.check(L.cvhip_mesh_cull(dev.handle, *surf, 0, dp(d_poly), n_poly, dp(d_keep), hp(stats)), "cull"))
        keep = d_keep.clone()
        if first_keep is None:
            first_keep = keep
        image_ms = best(lambda: _lib.check(L.cvhip_mesh_depth_image(
            dev.handle, *surf, 0, -1.0, dp(d_poly), n_poly, dp(d_map), d_map.numel(), C.byref(w), C.byref(h), hp(origin), hp(minmax),
            C.byref(wide)), "depth_image"))
        row = {"threshold": thr, "cull_camera0_ms": round(cull_ms, 3), "depth_image_ms": round(image_ms, 3),
               "cull_wide": [int(stats[j, 4]) for j in range(m)], "cull_dropped": [int(stats[j, 3]) for j in range(m)],
               "image_wide": int(wide.value), "kept": int(keep.sum().item()), "same_flags": bool(torch.equal(keep, first_keep))}
        result["sweep"].append(row)
        print(json.dumps(row), flush=True)
    mesh.set_wide_threshold(dev, mesh.WIDE_THRESHOLD_DEFAULT)
    result["stages_ms"] = {k_: round(v, 3) for k_, v in result["stages_ms"].items()}
    dev.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
