"""Times the OBJ writer (cvhip_mesh_obj) on bench_mesh.py's synthetic surface: size^2 tracks, 3 images, two
triangles per lattice cell, each polygon with the camera of its position in the list (three groups).  Per mode - Plain, Color,
Texture - the end-to-end time of the sizing call (cap = 0: the checks and the length pass) and of the whole call with the
output in device memory (host clock around the call: every entry synchronises), as median and spread over --repeat runs after
--warmup, with the sections' bytes.  Inputs are resident on the device.  For scale: cvhip_mesh_ply on the same surface, and one
host thread writing the Plain mode's v lines with the same formatter (tests/cpp/f64_display_host.cpp --time, built with g++ -O2:
the stand-in for the reference's serial write! loop).

Kernel times, and with them the rate of each section and the length pass's share, come from a kernel trace, taken in a run of
its own (tracing slows the host):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/tools/bench_mesh_obj.py --repeat 3
    python tests/tools/bench_mesh_obj.py --kernel-trace DIR --out profiles/x.json     # times again, adds the trace's medians

    python tests/tools/bench_mesh_obj.py [--size 2048] [--repeat 5] [--warmup 1] [--kernel-trace DIR] [--out profiles/x.json]
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import bench_mesh  # noqa: E402
from cybervision_amd import _lib, correlation, mesh  # noqa: E402

# kernel (name, template arguments) -> (mode whose section bytes it moves, section, pass)
KERNELS = {("mesh_obj_vertex_kernel", "<false, false>"): ("plain", "v", "length"), ("mesh_obj_vertex_kernel", "<false, true>"): ("plain", "v", "write"),
           ("mesh_obj_vertex_kernel", "<true, false>"): ("color", "v", "length"), ("mesh_obj_vertex_kernel", "<true, true>"): ("color", "v", "write"),
           ("mesh_obj_uv_kernel", "<false>"): ("texture", "vt", "length"), ("mesh_obj_uv_kernel", "<true>"): ("texture", "vt", "write"),
           ("mesh_obj_face_kernel", "<false, false>"): ("plain", "f", "length"), ("mesh_obj_face_kernel", "<false, true>"): ("plain", "f", "write"),
           ("mesh_obj_face_kernel", "<true, false>"): ("texture", "f", "length"), ("mesh_obj_face_kernel", "<true, true>"): ("texture", "f", "write"),
           ("mesh_obj_count_kernel", ""): (None, "count", "length"), ("mesh_obj_uv_index_kernel", ""): (None, "uv_index", "length"),
           ("obj_scan_u64_kernel", ""): (None, "scan", "length")}


def kernel_medians(trace_dir, sections):
    """-> {"kernel<args>": {"median_us", "launches", "section", "pass", "gb_per_s"}} from rocprofv3's *kernel_trace.csv"""
    spans = {k: [] for k in KERNELS}
    for f in glob.glob(f"{trace_dir}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            for k in KERNELS:
                if k[0] in r["Kernel_Name"] and k[1] in r["Kernel_Name"]:
                    spans[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for k, v in spans.items():
        if not v:
            continue
        mode, section, which = KERNELS[k]
        row = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "launches": len(v), "section": section, "pass": which}
        if mode:
            row["gb_per_s"] = round(sections[mode][section] / row["median_us"] / 1e3, 2)
        out[k[0] + k[1]] = row
    return out


def host_loop(values):
    """seconds one host thread takes to write "v x y z\\n" for each three doubles with f64_display.hpp"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = Path(tmp) / "f64_display_host"
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "cpp" / "f64_display_host.cpp")])
        values.tofile(Path(tmp) / "values.bin")
        runs = [json.loads(subprocess.run([str(exe), "--time", str(Path(tmp) / "values.bin")], capture_output=True, text=True, check=True).stdout)
                for _ in range(3)]
    best = min(runs, key=lambda r: r["seconds"])
    return {"lines": best["lines"], "bytes": best["bytes"], "ms": round(best["seconds"] * 1e3, 2),
            "gb_per_s": round(best["bytes"] / best["seconds"] / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    size = args.size
    X, tracks, _P, _r, _t, _dims, polygons, _n_long = bench_mesh.build_surface(size)
    n, n_poly, m = len(X), len(polygons), 3
    rng = np.random.default_rng(2)
    images = [rng.integers(0, 256, (size, size - size // 10, 3), dtype=np.uint8) for _ in range(m)]
    first = np.where((tracks[:, :, 0] >= 0).any(axis=1), (tracks[:, :, 0] >= 0).argmax(axis=1), 0)
    tracks[np.arange(n), first] = np.maximum(tracks[np.arange(n), first], 0)  # (every track has a point: Color and Texture require it)
    cameras = (np.arange(n_poly, dtype=np.uint64) * m // max(n_poly, 1)).astype(np.uint32)
    img_args, _keep = mesh._image_args(images)
    dev = correlation.create_gpu_context()
    L = _lib.lib()
    d_pts, d_tracks = torch.from_numpy(X).cuda(), torch.from_numpy(tracks).cuda()
    d_poly, d_cam = torch.from_numpy(polygons.view(np.int32)).cuda(), torch.from_numpy(cameras.view(np.int32)).cuda()
    d_img = torch.from_numpy(_keep[0]).cuda()
    scale = np.array([1.0, 1.0, -1.0])
    dp = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    size_out, sec = C.c_uint64(0), np.zeros(4, dtype=np.uint64)

    def obj_call(mode, out, cap):
        _lib.check(L.cvhip_mesh_obj(dev.handle, dp(d_pts), dp(d_tracks), n, m, dp(d_img), img_args[1], img_args[2], mode, hp(scale), dp(d_poly),
                                    dp(d_cam), n_poly, b"bench", out, cap, C.byref(size_out), hp(sec)), "cvhip_mesh_obj")

    def ply_call(mode, out, cap):
        _lib.check(L.cvhip_mesh_ply(dev.handle, dp(d_pts), dp(d_tracks), n, m, dp(d_img), img_args[1], img_args[2], mode, hp(scale), dp(d_poly),
                                    n_poly, out, cap, C.byref(size_out), hp(sec)), "cvhip_mesh_ply")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    result = {"size": size, "tracks": n, "polygons": n_poly, "images": m, "repeat": args.repeat, "warmup": args.warmup,
              "device": dev.name(), "obj": {}, "ply": {}}
    for call, key, names in ((obj_call, "obj", ("header", "v", "vt", "f")), (ply_call, "ply", ("header", "vertices", "faces"))):
        for mode, name in enumerate(("plain", "color", "texture")):
            if key == "ply" and name == "texture":
                continue
            call(mode, None, 0)
            total = size_out.value
            row = {"file_bytes": total, **{s: int(v) for s, v in zip(names, sec)}}
            d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()  # (torch works on its own stream, the library on the handle's)
            row["sizing_call"] = timed(lambda: call(mode, None, 0))
            row["device_out"] = timed(lambda: call(mode, dp(d_out), total))
            row["device_out"]["gb_per_s"] = round(total / row["device_out"]["median_ms"] / 1e6, 2)
            result[key][name] = row
            print(json.dumps({key + "_" + name: row}), flush=True)
            del d_out
    result["host_loop_plain_v"] = host_loop(np.ascontiguousarray(X * scale * np.array([1.0, -1.0, 1.0])))
    print(json.dumps({"host_loop_plain_v": result["host_loop_plain_v"]}), flush=True)
    if args.kernel_trace:
        result["kernels"] = kernel_medians(args.kernel_trace, result["obj"])
    dev.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
