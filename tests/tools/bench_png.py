"""Times the PNG encoder (cvhip_png_encode) on the two images the mesh output saves, at size^2: a texture-like RGB
image (a smooth surface, an edge pattern and two bits of noise) and a depth-map-like RGBA image (a colour ramp over a smooth
depth with a transparent border).  Per image the end-to-end time of the sizing call (cap = 0: filter, count, the code from the
host, the rows' bits, the scan) and of the whole call with pixels and output in device memory (host clock around the call: the
entry synchronises), as median and spread over --repeat runs after --warmup, with the file's size; Pillow must open the file to
the pixels.  For scale, not a gate: one host thread running zlib.compress(filtered bytes, 1) - the filtered bytes are given, the
filter's time is not counted - and Pillow's save of the same pixels.

Kernel times per pass come from a kernel trace, taken in a run of its own (tracing slows the host):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/tools/bench_png.py --repeat 3
    python tests/tools/bench_png.py --kernel-trace DIR --out profiles/x.json     # times again, adds the trace's medians

    python tests/tools/bench_png.py [--size 2048] [--image both|texture_rgb|depth_rgba] [--repeat 5] [--warmup 1] [--kernel-trace DIR]
                                    [--out profiles/x.json]
    python tests/tools/bench_png.py --summarise DIR          # a trace's medians alone (no GPU): one trace per --image tells them apart
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
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ref_png  # noqa: E402
from cybervision_amd import _lib, correlation, mesh  # noqa: E402

KERNELS = ("png_filter_kernel", "png_histogram_kernel", "png_length_kernel", "obj_scan_u64_kernel", "png_write_kernel", "png_trailer_kernel",
           "png_crc_kernel", "png_finish_kernel")


def texture(size):
    rng = np.random.default_rng(4)
    y, x = np.mgrid[0:size, 0:size]
    base = 128 + 70 * np.sin(x / 97.0) * np.cos(y / 61.0) + 30 * ((x // 64 + y // 64) % 2)
    img = base[:, :, None] + np.array([0.0, 11.0, -17.0])[None, None, :] + rng.integers(0, 4, (size, size, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def depth_map(size):
    y, x = np.mgrid[0:size, 0:size]
    depth = 0.5 + 0.5 * np.sin(x / 211.0) * np.cos(y / 173.0)
    idx = np.clip(depth * 255, 0, 255).astype(np.int64)
    table = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 3) % 256], axis=1)
    rgba = np.concatenate([table[idx], np.full((size, size, 1), 255)], axis=2).astype(np.uint8)
    r = np.hypot(x - size / 2, y - size / 2)
    rgba[r > size * 0.47] = 0  # cells without a depth
    return rgba


def kernel_medians(trace_dir):
    """-> {kernel: {"median_us", "min_us", "launches"}} from rocprofv3's *kernel_trace.csv"""
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
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--image", default="both", choices=("both", "texture_rgb", "depth_rgba"))
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

    result = {"size": args.size, "repeat": args.repeat, "warmup": args.warmup, "device": dev.name(), "images": {}}
    for name, make in (("texture_rgb", texture), ("depth_rgba", depth_map)):
        if args.image not in ("both", name):
            continue
        pixels = make(args.size)
        h, w, c = pixels.shape
        d_pixels = torch.from_numpy(pixels).cuda()

        def call(out, cap):
            _lib.check(L.cvhip_png_encode(dev.handle, C.c_void_p(d_pixels.data_ptr()), w, h, c, int(mesh.PngFilter.Adaptive), out, cap,
                                          C.byref(size_out), C.c_void_p(sec.ctypes.data)), "cvhip_png_encode")

        torch.cuda.synchronize()  # (torch works on its own stream, the library on the handle's)
        call(None, 0)
        total = size_out.value
        d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        row = {"pixel_bytes": int(pixels.size), "file_bytes": total, "idat_bytes": int(sec[1])}
        row["sizing_call"] = timed(lambda: call(None, 0))
        row["device_out"] = timed(lambda: call(C.c_void_p(d_out.data_ptr()), total))
        row["device_out"]["pixel_gb_per_s"] = round(pixels.size / row["device_out"]["median_ms"] / 1e6, 2)
        file = d_out.cpu().numpy().tobytes()
        if not (np.asarray(Image.open(io.BytesIO(file))) == pixels).all():
            raise SystemExit(f"{name}: Pillow does not open the file to the pixels")
        # for scale: one host thread, the filtered bytes given
        filtered = zlib.decompress(file[41:41 + int(sec[1])])
        assert len(filtered) == h * (1 + w * c)
        t0 = time.perf_counter()
        packed = zlib.compress(filtered, 1)
        row["host_zlib_level_1"] = {"ms": round((time.perf_counter() - t0) * 1e3, 2), "bytes": len(packed)}
        row["stored_blocks_bytes"] = ref_png.stored_size(len(filtered))
        buf = io.BytesIO()
        t0 = time.perf_counter()
        Image.fromarray(pixels).save(buf, format="PNG")
        row["host_pillow_save"] = {"ms": round((time.perf_counter() - t0) * 1e3, 2), "bytes": len(buf.getvalue())}
        result["images"][name] = row
        print(json.dumps({name: row}), flush=True)
        del d_out, d_pixels
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
