"""Times the JPEG decoder (cvhip_jpeg_decode) on two files at size^2, both quality 90 without DRI: a photo-like
colour file at 4:2:0 (synth's value-noise texture per channel, rectangles and two bits of noise) and the grey file of its
first channel.  Per file and format the end-to-end time of the sizing call (cap = 0: the host's marker walk alone) and of the
whole call with `out` in device memory (host clock around the call: the entry synchronises), as median and spread over
--repeat runs after --warmup, with the synchronisation's counts (cvhip_jpeg_last_stats); the RGB8 must equal Pillow's.  For
scale, not a gate: one host thread of Pillow (libjpeg-turbo) decoding the same bytes to RGB and to L.

Kernel times per pass come from a kernel trace, taken in a run of its own (tracing slows the host):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/tools/bench_jpeg.py --repeat 3 --file colour_420
    python tests/tools/bench_jpeg.py --summarise DIR          # a trace's medians alone (no GPU)

    python tests/tools/bench_jpeg.py [--size 2048] [--file both|colour_420|grey] [--repeat 7] [--warmup 2] [--kernel-trace DIR]
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

from cybervision_amd import _lib, correlation, image, synth  # noqa: E402

KERNELS = ("jpeg_mark_kernel", "jpeg_compact_kernel", "jpeg_segments_kernel", "jpeg_sync_kernel", "jpeg_write_kernel", "jpeg_dc_kernel",
           "jpeg_idct_kernel", "jpeg_pixels_kernel", "obj_scan_u64_kernel")


def photo(size):
    rng = np.random.default_rng(9)
    xs = np.arange(size, dtype=np.int64)[None, :]
    ys = np.arange(size, dtype=np.int64)[:, None]
    channels = []
    for seed in (1234, 77, 4321):
        canvas = np.clip(synth.texture(xs, ys, seed), 0, 255).astype(np.uint8)
        channels.append(synth.add_blocks(canvas, count=max(size * size // 2600, 40), seed=seed + 70))
    img = np.stack(channels, axis=2).astype(np.int64) + rng.integers(0, 4, (size, size, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def kernel_totals(trace_dir):
    """-> {kernel: {"median_us", "min_us", "max_us", "launches"}} from rocprofv3's *kernel_trace.csv"""
    spans = {k: [] for k in KERNELS}
    for f in glob.glob(f"{trace_dir}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    spans[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "launches": len(v)}
            for k, v in spans.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--file", default="both", choices=("both", "colour_420", "grey"))
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise:
        print(json.dumps({"kernels": kernel_totals(args.summarise)}))
        return
    import torch
    from PIL import Image

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

    pixels = photo(args.size)
    result = {"size": args.size, "repeat": args.repeat, "warmup": args.warmup, "device": dev.name(), "files": {}}
    for name in ("colour_420", "grey"):
        if args.file not in ("both", name):
            continue
        buf = io.BytesIO()
        Image.fromarray(pixels if name == "colour_420" else pixels[:, :, 0]).save(buf, format="JPEG", quality=90,
                                                                                   **({"subsampling": 2} if name == "colour_420" else {}))
        data = buf.getvalue()
        file = np.frombuffer(data, dtype=np.uint8)
        row = {"file_bytes": len(data), "info": image.jpeg_info(data)}
        for mode, fmt, channels in (("rgb8", image.RGB8, 3), ("luma8", image.LUMA8, 1)):
            d_out = torch.empty(args.size * args.size * channels, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()  # (torch works on its own stream, the library on the handle's)

            def call(out, cap):
                _lib.check(L.cvhip_jpeg_decode(dev.handle, C.c_void_p(file.ctypes.data), len(data), fmt, 0, out, cap, C.byref(size_out)),
                           "cvhip_jpeg_decode")

            row[mode] = {"sizing_call": timed(lambda: call(None, 0)), "device_out": timed(lambda: call(C.c_void_p(d_out.data_ptr()), d_out.numel()))}
            row[mode]["device_out"]["pixel_gb_per_s"] = round(d_out.numel() / row[mode]["device_out"]["median_ms"] / 1e6, 2)
            row[mode]["sync"] = image.jpeg_last_stats()
            got = d_out.cpu().numpy()
            t0 = time.perf_counter()
            want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB" if channels == 3 else "L"))
            row[mode]["host_pillow_one_thread_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            if channels == 3 and not (got.reshape(want.shape) == want).all():
                raise SystemExit(f"{name}: the RGB8 is not Pillow's")
            del d_out
        result["files"][name] = row
        print(json.dumps({name: row}), flush=True)
    if args.kernel_trace:
        result["kernels"] = kernel_totals(args.kernel_trace)
    dev.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
