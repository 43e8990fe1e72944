"""Times the TIFF decoder (cvhip_tiff_decode) on files of Pillow's (libtiff's) at size^2 of a photo-like picture
(bench_jpeg.py's): 8-bit grey uncompressed; 8-bit grey LZW in libtiff's 64 KB strips; 16-bit grey LZW with Predictor 2; RGB8
PackBits; and the grey LZW picture as ONE strip, which decodes on one wave (correct and slow: written down, not engineered
around).  Per file the end-to-end time of the sizing call (cap = 0: the host's IFD walk alone) and of the whole call to its
natural format with `out` in device memory (host clock around the call: the entry synchronises), as median and spread over
--repeat runs after --warmup, with the decompression's counts (cvhip_tiff_last_stats); the pixels must equal Pillow's.  For
scale, not a gate: one host thread of Pillow opening the same bytes.

Kernel times come from a kernel trace, taken in a run of its own per file (tracing slows the host):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/tools/bench_tiff.py --repeat 3 --file grey8_lzw
    python tests/tools/bench_tiff.py --summarise DIR          # a trace's medians alone (no GPU)

    python tests/tools/bench_tiff.py [--size 2048] [--file all|NAME] [--repeat 7] [--warmup 2] [--out profiles/x.json]
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

from bench_jpeg import photo  # noqa: E402
from cybervision_amd import _lib, correlation, image  # noqa: E402


def pillow_tiff(a, compression, predictor=False, strip_rows=None):
    from PIL import Image, TiffImagePlugin

    info = TiffImagePlugin.ImageFileDirectory_v2()
    if predictor:
        info[317] = 2
    if strip_rows is not None:
        info[278] = strip_rows
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="TIFF", compression=compression, tiffinfo=info)
    return buf.getvalue()


KERNELS = ("tiff_lzw_kernel", "tiff_packbits_kernel", "tiff_convert_kernel")


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
    ap.add_argument("--file", default="all")
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
    grey = pixels[:, :, 0]
    grey16 = (grey.astype(np.uint32) * 257 + (pixels[:, :, 1] & 63)).clip(0, 65535).astype(np.uint16)   # (low bits that are not the high byte's)
    files = (("grey8_raw", lambda: pillow_tiff(grey, "raw"), image.LUMA8), ("grey8_lzw", lambda: pillow_tiff(grey, "tiff_lzw"), image.LUMA8),
             ("grey16_lzw_predictor", lambda: pillow_tiff(grey16, "tiff_lzw", True), image.LUMA8),
             ("rgb8_packbits", lambda: pillow_tiff(pixels, "packbits"), image.RGB8),
             ("grey8_lzw_one_strip", lambda: pillow_tiff(grey, "tiff_lzw", strip_rows=args.size), image.LUMA8))
    result = {"size": args.size, "repeat": args.repeat, "warmup": args.warmup, "device": dev.name(), "files": {}}
    for name, make, fmt in files:
        if args.file not in ("all", name):
            continue
        data = make()
        file = np.frombuffer(data, dtype=np.uint8)
        info = image.tiff_info(data)
        channels = 3 if fmt == image.RGB8 else 1
        d_out = torch.empty(args.size * args.size * channels, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (torch works on its own stream, the library on the handle's)

        def call(out, cap):
            _lib.check(L.cvhip_tiff_decode(dev.handle, C.c_void_p(file.ctypes.data), len(data), fmt, 0, out, cap, C.byref(size_out)), "cvhip_tiff_decode")

        row = {"file_bytes": len(data), "strips": info["strips"], "bits": info["bits"], "samples": info["samples"],
               "sizing_call": timed(lambda: call(None, 0)), "device_out": timed(lambda: call(C.c_void_p(d_out.data_ptr()), d_out.numel()))}
        row["device_out"]["pixel_gb_per_s"] = round(d_out.numel() / row["device_out"]["median_ms"] / 1e6, 2)
        row["stats"] = image.tiff_last_stats()
        got = d_out.cpu().numpy()
        t0 = time.perf_counter()
        want = np.asarray(Image.open(io.BytesIO(data)))
        row["host_pillow_one_thread_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        if want.dtype != np.uint8:
            want = ((want.astype(np.uint32) + 128) // 257).astype(np.uint8)
        if not (got.reshape(want.shape) == want).all():
            raise SystemExit(f"{name}: the pixels are not Pillow's")
        del d_out
        result["files"][name] = row
        print(json.dumps({name: row}), flush=True)
    dev.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
