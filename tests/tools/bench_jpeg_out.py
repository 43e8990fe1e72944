"""Times the JPEG encoder (cvhip_jpeg_encode) at size^2 with pixels and output in device memory: a texture-like
RGB image (a smooth surface, an edge pattern and two bits of noise) at 4:2:0 and 4:4:4, quality 90, and a depth-map-like RGBA
image (a colour ramp over a smooth depth with a border without depth) at 4:2:0, quality 75 - each with and without optimize.
Per case the end-to-end time of the sizing call (cap = 0: everything but the last copy) and of the whole call (host clock
around the call: the entry synchronises), as median and spread over --repeat runs after --warmup, with the file's size and
cvhip_jpeg_encode_last_stats; the file must equal Pillow's save of the same pixels (the RGB part of the RGBA image) byte for
byte.  For scale, not a gate: one host thread of Pillow's save on the same pixels.

The split over the five stages (transform, lengths, scan, write, stuffing) comes from a kernel trace, taken in a run of its own
(tracing slows the host):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/tools/bench_jpeg_out.py --repeat 3
    python tests/tools/bench_jpeg_out.py --kernel-trace DIR --out profiles/x.json     # times again, adds the trace's medians

    python tests/tools/bench_jpeg_out.py [--size 2048] [--repeat 5] [--warmup 1] [--kernel-trace DIR] [--out profiles/x.json]
    python tests/tools/bench_jpeg_out.py --summarise DIR          # a trace's medians alone (no GPU)
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import io
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "tools"))

from bench_png import depth_map, texture  # noqa: E402  (the two images the mesh output saves)
from cybervision_amd import _lib, correlation, mesh  # noqa: E402

# kernel -> stage
STAGES = {"jpeg_transform_kernel": "transform", "jpeg_dummy_dc_kernel": "transform", "jpeg_entropy_kernel": "lengths",
          "obj_scan_u64_kernel": "scan", "jpeg_write_kernel": "write", "jpeg_stuff_count_kernel": "stuffing",
          "jpeg_stuff_copy_kernel": "stuffing"}
CASES = (("texture_rgb_420_q90", texture, 90, 2), ("texture_rgb_444_q90", texture, 90, 0), ("depth_rgba_420_q75", depth_map, 75, 2))


def kernel_medians(trace_dir):
    """-> {kernel: {"median_us", "min_us", "max_us", "launches", "stage"}} from rocprofv3's *kernel_trace.csv (all cases together:
    trace one case with --case to tell them apart)"""
    spans = {k: [] for k in STAGES}
    for f in glob.glob(f"{trace_dir}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            for k in STAGES:
                if k in r["Kernel_Name"]:
                    spans[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "launches": len(v),
                "stage": STAGES[k]} for k, v in spans.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case", default="all", choices=("all",) + tuple(c[0] for c in CASES))
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise:
        print(json.dumps({"kernels": kernel_medians(args.summarise)}))
        return
    import torch
    from PIL import Image

    dev = correlation.create_gpu_context()
    L = _lib.lib()
    size_out, sec = C.c_uint64(0), np.zeros(3, dtype=np.uint64)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    result = {"size": args.size, "repeat": args.repeat, "warmup": args.warmup, "device": dev.name(), "cases": {}}
    for name, make, quality, sampling in CASES:
        if args.case not in ("all", name):
            continue
        pixels = make(args.size)
        h, w, c = pixels.shape
        d_pixels = torch.from_numpy(pixels).cuda()
        torch.cuda.synchronize()  # (torch works on its own stream, the library on the handle's)
        for optimize in (0, 1):
            def call(out, cap):
                _lib.check(L.cvhip_jpeg_encode(dev.handle, C.c_void_p(d_pixels.data_ptr()), w, h, c, quality, sampling, optimize, out, cap,
                                               C.byref(size_out), C.c_void_p(sec.ctypes.data)), "cvhip_jpeg_encode")

            call(None, 0)
            total = size_out.value
            d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            row = {"pixel_bytes": int(pixels.size), "file_bytes": total, "data_bytes": int(sec[1])}
            row["sizing_call"] = timed(lambda: call(None, 0))
            row["device_out"] = timed(lambda: call(C.c_void_p(d_out.data_ptr()), total))
            row["device_out"]["pixel_gb_per_s"] = round(pixels.size / row["device_out"]["median_ms"] / 1e6, 2)
            row["stats"] = mesh.jpeg_encode_last_stats()
            file = d_out.cpu().numpy().tobytes()
            buf = io.BytesIO()
            t0 = time.perf_counter()
            Image.fromarray(pixels[..., :3]).save(buf, format="JPEG", quality=quality, subsampling=sampling, optimize=bool(optimize))
            row["host_pillow_save"] = {"ms": round((time.perf_counter() - t0) * 1e3, 2), "bytes": len(buf.getvalue())}
            if file != buf.getvalue():
                raise SystemExit(f"{name}: the file is not Pillow's")
            key = name + ("_optimize" if optimize else "")
            result["cases"][key] = row
            print(json.dumps({key: row}), flush=True)
            del d_out
        del d_pixels
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
