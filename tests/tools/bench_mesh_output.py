"""Times the mesh output (cvhip_mesh_ply, cvhip_mesh_colour_map) on bench_mesh.py's synthetic surface:
size^2 tracks, 3 images, two triangles per lattice cell.  Per section - the vertices in Plain mode, the vertices in Color
mode, the faces, the colour map of a size^2 depth map - the end-to-end time of the call (host clock around it: every entry
synchronises) with the output in device memory and in pageable host memory, as median and spread over --repeat runs after
--warmup, and the section's bytes over the median.  Inputs are resident on the device.

A section is a call of its own: the vertices with an empty polygon list, the faces with a 256-track surface (their
vertices folded onto it; 6 KB of vertex records against 109 MB of faces).

Kernel times come from a kernel trace, taken in a run of its own (tracing slows the host):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/tools/bench_mesh_output.py --repeat 5
    python tests/tools/bench_mesh_output.py --kernel-trace DIR --out profiles/x.json     # times again, adds the trace's medians

    python tests/tools/bench_mesh_output.py [--size 2048] [--repeat 9] [--warmup 2] [--kernel-trace DIR] [--out profiles/x.json]
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
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

KERNELS = ("mesh_ply_vertex_kernel<true, false>", "mesh_ply_vertex_kernel<false, true>", "mesh_ply_vertex_kernel<true, true>",
           "mesh_ply_face_kernel", "mesh_colour_kernel")


def kernel_medians(trace_dir):
    """-> {kernel: {"median_us", "min_us", "max_us", "launches"}} from rocprofv3's *kernel_trace.csv under trace_dir"""
    spans = {k: [] for k in KERNELS}
    for f in glob.glob(f"{trace_dir}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            for k in KERNELS:
                if k.split("<")[0] in r["Kernel_Name"] and (("<" not in k) or k.split("<")[1] in r["Kernel_Name"]):
                    spans[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "launches": len(v)}
            for k, v in spans.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    size = args.size
    X, tracks, _P, _r, _t, _dims, polygons, _n_long = bench_mesh.build_surface(size)
    n, n_poly, m = len(X), len(polygons), 3
    rng = np.random.default_rng(2)
    # images a tenth narrower than the tracks' range: about a tenth of the first points get no colour bytes
    images = [rng.integers(0, 256, (size, size - size // 10, 3), dtype=np.uint8) for _ in range(m)]
    first = np.where((tracks[:, :, 0] >= 0).any(axis=1), (tracks[:, :, 0] >= 0).argmax(axis=1), 0)
    tracks[np.arange(n), first] = np.maximum(tracks[np.arange(n), first], 0)  # (every track has a point: Color mode requires it)
    img_args, _keep = mesh._image_args(images)
    depth = 5.0 + np.sin(np.arange(size * size, dtype=np.float64) * 1e-3).reshape(size, size)
    depth[rng.random(depth.shape) < 0.1] = np.nan
    table = np.stack([(37 * np.arange(256) + 11) % 256, (101 * np.arange(256) + 7) % 256, (201 * np.arange(256)) % 256], axis=1).astype(np.uint8)
    dev = correlation.create_gpu_context()
    L = _lib.lib()
    d_pts, d_tracks = torch.from_numpy(X).cuda(), torch.from_numpy(tracks).cuda()
    d_poly = torch.from_numpy(polygons.view(np.int32)).cuda()
    d_poly_folded = torch.from_numpy((polygons % 256).astype(np.uint32).view(np.int32)).cuda()
    d_img = torch.from_numpy(_keep[0]).cuda()
    d_depth = torch.from_numpy(depth).cuda()
    scale = np.array([1.0, 1.0, -1.0])
    dp = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    size_out, sec = C.c_uint64(0), np.zeros(3, dtype=np.uint64)

    def ply_call(n_tracks, mode, poly, k, out, cap):
        _lib.check(L.cvhip_mesh_ply(dev.handle, dp(d_pts), dp(d_tracks), n_tracks, m, dp(d_img), img_args[1], img_args[2], mode, hp(scale),
                                    dp(poly) if k else None, k, out, cap, C.byref(size_out), hp(sec)), "cvhip_mesh_ply")

    sections = {"vertex_plain": (n, 0, d_poly, 0, 1), "vertex_color": (n, 1, d_poly, 0, 1), "face": (256, 0, d_poly_folded, n_poly, 2)}
    result = {"size": size, "tracks": n, "polygons": n_poly, "images": m, "repeat": args.repeat, "warmup": args.warmup,
              "device": dev.name(), "sections": {}}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    for name, (n_tracks, mode, poly, k, which) in sections.items():
        ply_call(n_tracks, mode, poly, k, None, 0)
        total, moved = size_out.value, int(sec[which])
        d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
        h_out = np.empty(total, dtype=np.uint8)
        torch.cuda.synchronize()  # (torch works on its own stream, the library on the handle's)
        row = {"bytes": moved, "file_bytes": total,
               "sizing_call": timed(lambda: ply_call(n_tracks, mode, poly, k, None, 0)),
               "device_out": timed(lambda: ply_call(n_tracks, mode, poly, k, dp(d_out), total)),
               "host_out": timed(lambda: ply_call(n_tracks, mode, poly, k, hp(h_out), total))}
        for where in ("device_out", "host_out"):
            row[where]["gb_per_s"] = round(moved / row[where]["median_ms"] / 1e6, 2)
        assert d_out.cpu().numpy().tobytes() == h_out.tobytes()
        result["sections"][name] = row
        print(json.dumps({name: row}), flush=True)
        del d_out, h_out
    d_rgba = torch.empty((size, size, 4), dtype=torch.uint8, device="cuda")
    h_rgba = np.empty((size, size, 4), dtype=np.uint8)
    lo, hi = float(np.nanmin(depth)), float(np.nanmax(depth))
    torch.cuda.synchronize()

    def colour_call(out):
        _lib.check(L.cvhip_mesh_colour_map(dev.handle, dp(d_depth), size, size, lo, hi, hp(table), out), "cvhip_mesh_colour_map")

    row = {"bytes": depth.nbytes + h_rgba.nbytes, "device_out": timed(lambda: colour_call(dp(d_rgba))), "host_out": timed(lambda: colour_call(hp(h_rgba)))}
    for where in ("device_out", "host_out"):
        row[where]["gb_per_s"] = round(row["bytes"] / row[where]["median_ms"] / 1e6, 2)
    assert d_rgba.cpu().numpy().tobytes() == h_rgba.tobytes()
    result["sections"]["colour_map"] = row
    print(json.dumps({"colour_map": row}), flush=True)
    if args.kernel_trace:
        result["kernels"] = kernel_medians(args.kernel_trace)
    dev.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
