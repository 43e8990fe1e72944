"""Times the progressive JPEG decoder (cvhip_jpeg_progressive_decode) on the photo-like picture of
tests/tools/bench_jpeg.py at size^2, quality 90, 4:2:0, written progressive by Pillow (libjpeg's default script), with `out`
in device memory: per format the end-to-end time of the sizing call (cap = 0: the host's walk over the whole file) and of the
whole call (host clock around the call: the entry synchronises), as median and spread over --repeat runs after --warmup, with
the counts of cvhip_jpeg_progressive_last_stats; the RGB8 must equal Pillow's.  For scale, not a gate: the baseline decoder
on the same picture written sequentially, and one host thread of Pillow (libjpeg-turbo) on the progressive file.

Kernel times come from a kernel trace, taken in a run of its own (tracing slows the host): per kernel the median launch and
the sum per decode; the AC-refinement launches (jpeg_prog_refine_kernel) are listed one by one in launch order with the scans
each holds:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/tools/bench_jpeg_prog.py --repeat 3 --mode rgb8
    python tests/tools/bench_jpeg_prog.py --summarise DIR          # a trace's medians alone (no GPU)

    python tests/tools/bench_jpeg_prog.py [--size 2048] [--mode both|rgb8|luma8] [--repeat 7] [--warmup 2] [--kernel-trace DIR]
                                          [--out profiles/x.json]
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
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "tools"))

import bench_jpeg  # noqa: E402
import ref_jpeg_prog  # noqa: E402

KERNELS = ("jpeg_prog_mark_kernel", "jpeg_prog_compact_kernel", "jpeg_prog_segments_kernel", "jpeg_prog_subseq_kernel", "jpeg_prog_sync_kernel",
           "jpeg_prog_write_kernel", "jpeg_prog_dc_sums_kernel", "jpeg_prog_dc_values_kernel", "jpeg_prog_dc_refine_kernel", "jpeg_prog_dc_kernel",
           "jpeg_idct_kernel", "jpeg_pixels_kernel", "obj_scan_u64_kernel")
REFINE = "jpeg_prog_refine_kernel"


def progressive_file(size):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(bench_jpeg.photo(size)).save(buf, format="JPEG", quality=90, subsampling=2, progressive=True)
    return buf.getvalue()


def launches_of(data):
    """The launches of jpeg_prog_refine_kernel in order, as the host orders them (jpeg_prog_common.hpp: a refinement lies
    behind every earlier scan of its component whose band overlaps its own; a level's AC-refinement scans go in one launch)
    -> per launch the scans it holds; and the first scans, which settle together."""
    scans = ref_jpeg_prog.parse(data)["scans"]
    levels = []
    for k, b in enumerate(scans):
        level = 0
        if b["ah"]:
            for a, la in zip(scans[:k], levels):
                if set(a["comps"]) & set(b["comps"]) and a["ss"] <= b["se"] and b["ss"] <= a["se"]:
                    level = max(level, la + 1)
        levels.append(level)

    def name(s):
        return "%s %d-%d Ah%d Al%d %dB" % ("".join("YBR"[c] for c in s["comps"]), s["ss"], s["se"], s["ah"], s["al"], s["range"][1] - s["range"][0])

    out = {"first_scans": [name(s) for s in scans if s["ah"] == 0], "dc_refinements": [name(s) for s in scans if s["ah"] and s["ss"] == 0], REFINE: []}
    for level in range(max(levels) + 1):
        mine = [name(s) for s, lv in zip(scans, levels) if lv == level and s["ss"] > 0 and s["ah"] > 0]
        if mine:
            out[REFINE].append({"level": level, "scans": mine})
    return out


def kernel_totals(trace_dir, launches):
    """-> {kernel: medians over all its launches, launches per decode} and the AC-refinement launches (jpeg_prog_refine_kernel's)
    one by one in order, from rocprofv3's *kernel_trace.csv"""
    spans = {k: [] for k in KERNELS + (REFINE,)}
    for f in glob.glob(f"{trace_dir}/**/*kernel_trace.csv", recursive=True):
        for r in sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"])):
            for k in spans:
                if k in r["Kernel_Name"]:
                    spans[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)

    def medians(v):
        return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}

    decodes = max(len(spans["jpeg_pixels_kernel"]), 1)
    out = {k: {**medians(spans[k]), "launches_per_decode": round(len(spans[k]) / decodes, 2), "sum_us_per_decode": round(sum(spans[k]) / decodes, 2)}
           for k in KERNELS if spans[k]}
    for kernel in (REFINE,):
        v, per = spans[kernel], len(launches[kernel])
        if v and per and len(v) % per == 0:
            rows = [{**launch, **medians(v[k::per])} for k, launch in enumerate(launches[kernel])]
            out[kernel] = {"launches_per_decode": per, "decodes": len(v) // per, "launches": rows, "median_us_sum": round(sum(r["median_us"] for r in rows), 2)}
        elif v:
            out[kernel] = {**medians(v), "launches": len(v)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mode", default="both", choices=("both", "rgb8", "luma8"))
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    data = progressive_file(args.size)
    launches = launches_of(data)
    if args.summarise:
        print(json.dumps({"kernels": kernel_totals(args.summarise, launches)}))
        return
    import torch
    from PIL import Image

    from cybervision_amd import _lib, correlation, image

    dev = correlation.create_gpu_context()
    L = _lib.lib()
    size_out = C.c_uint64(0)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    file = np.frombuffer(data, dtype=np.uint8)
    result = {"size": args.size, "repeat": args.repeat, "warmup": args.warmup, "device": dev.name(), "file_bytes": len(data),
              "info": image.jpeg_progressive_info(data), "launches": launches}
    for mode, fmt, channels in (("rgb8", image.RGB8, 3), ("luma8", image.LUMA8, 1)):
        if args.mode not in ("both", mode):
            continue
        d_out = torch.empty(args.size * args.size * channels, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (torch works on its own stream, the library on the handle's)

        def call(out, cap):
            _lib.check(L.cvhip_jpeg_progressive_decode(dev.handle, C.c_void_p(file.ctypes.data), len(data), fmt, 0, out, cap, C.byref(size_out)),
                       "cvhip_jpeg_progressive_decode")

        row = {"sizing_call": timed(lambda: call(None, 0)), "device_out": timed(lambda: call(C.c_void_p(d_out.data_ptr()), d_out.numel()))}
        row["stats"] = image.jpeg_progressive_last_stats()
        got = d_out.cpu().numpy()
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB" if channels == 3 else "L"))
            ms.append((time.perf_counter() - t0) * 1e3)
        row["host_pillow_one_thread_ms"] = round(statistics.median(ms), 2)
        if channels == 3 and not (got.reshape(want.shape) == want).all():
            raise SystemExit("the RGB8 is not Pillow's")
        del d_out
        result[mode] = row
        print(json.dumps({mode: row}), flush=True)
    if args.kernel_trace:
        result["kernels"] = kernel_totals(args.kernel_trace, launches)
    dev.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
