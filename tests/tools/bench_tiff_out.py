"""Times the TIFF encoder (cvhip_tiff_encode) at size^2 with pixels and output in device memory: the texture-like
RGB image and the depth-map-like RGBA image of bench_png.py, each uncompressed, as LZW with Predictor 2 and as PackBits, at the
default rows per strip.  Per case the end-to-end time of the sizing call (cap = 0: everything but the header, the two arrays
and the copy) and of the whole call (host clock around the call: the entry synchronises), as median and spread over --repeat
runs after --warmup, with the file's size and cvhip_tiff_encode_last_stats.  For LZW the shares of the kernel's time spent
loading, on the serial walk and packing (cvhip_tiff_encode_last_phases: ticks summed over the strips' waves) are reported
separately.  Every file must read back to the pixels (Pillow); every LZW strip must equal the strip Pillow (libtiff) writes.
For scale, not a gate: one host thread of Pillow's save on the same pixels.

The split over the kernels comes from a kernel trace, taken in a run of its own (tracing slows the host):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/tools/bench_tiff_out.py --repeat 3
    python tests/tools/bench_tiff_out.py --summarise DIR          # a trace's medians alone (no GPU)

    python tests/tools/bench_tiff_out.py [--size 2048] [--repeat 5] [--warmup 1] [--out profiles/x.json]
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

KERNELS = ("tiff_lzw_kernel", "tiff_packbits_kernel", "tiff_sizes_kernel", "obj_scan_u64_kernel", "tiff_table_kernel", "tiff_copy_kernel")
PICTURES = (("texture_rgb", texture), ("depth_rgba", depth_map))
COMPRESSIONS = (("none", 1, 1, "raw"), ("lzw_pred2", 5, 2, "tiff_lzw"), ("packbits", 32773, 1, "packbits"))


def kernel_medians(trace_dir):
    """-> {kernel: {"median_us", "min_us", "max_us", "launches"}} from rocprofv3's *kernel_trace.csv (all cases together)"""
    spans = {k: [] for k in KERNELS}
    for f in glob.glob(f"{trace_dir}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    spans[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "launches": len(v)}
            for k, v in spans.items() if v}


def strips(data):
    from PIL import Image

    tags = Image.open(io.BytesIO(data)).tag_v2
    return [data[o:o + n] for o, n in zip(tags[273], tags[279])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise:
        print(json.dumps({"kernels": kernel_medians(args.summarise)}))
        return
    import torch
    from PIL import Image, TiffImagePlugin

    dev = correlation.create_gpu_context()
    L = _lib.lib()
    size_out, sec, ticks = C.c_uint64(0), np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64)

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
    for pname, make in PICTURES:
        pixels = make(args.size)
        h, w, c = pixels.shape
        d_pixels = torch.from_numpy(pixels).cuda()
        torch.cuda.synchronize()  # (torch works on its own stream, the library on the handle's)
        for cname, compression, predictor, pillow_name in COMPRESSIONS:
            def call(out, cap):
                _lib.check(L.cvhip_tiff_encode(dev.handle, C.c_void_p(d_pixels.data_ptr()), w, h, c, compression, predictor, 0, out, cap,
                                               C.byref(size_out), C.c_void_p(sec.ctypes.data)), "cvhip_tiff_encode")

            call(None, 0)
            total = size_out.value
            d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            row = {"pixel_bytes": int(pixels.size), "file_bytes": total, "strip_bytes": int(sec[1])}
            row["sizing_call"] = timed(lambda: call(None, 0))
            row["device_out"] = timed(lambda: call(C.c_void_p(d_out.data_ptr()), total))
            row["device_out"]["pixel_gb_per_s"] = round(pixels.size / row["device_out"]["median_ms"] / 1e6, 2)
            row["stats"] = mesh.tiff_encode_last_stats()
            if compression == 5:
                _lib.check(L.cvhip_tiff_encode_last_phases(C.c_void_p(ticks.ctypes.data)), "cvhip_tiff_encode_last_phases")
                whole = float(ticks.sum())
                row["lzw_kernel_shares"] = {k: round(float(v) / whole, 4) for k, v in zip(("load", "serial_parse", "packing"), ticks)}
                row["lzw_wave_ms_per_strip"] = {k: round(float(v) / 1e5 / row["stats"]["strips"], 4)
                                                for k, v in zip(("load", "serial_parse", "packing"), ticks)}
            file = d_out.cpu().numpy().tobytes()
            opened = np.asarray(Image.open(io.BytesIO(file)))
            if opened.shape != pixels.shape or not (opened == pixels).all():
                raise SystemExit(f"{pname} {cname}: the file does not read back to the pixels")
            info = TiffImagePlugin.ImageFileDirectory_v2()
            info[278] = max(1, 8192 // (w * c))
            if predictor == 2:
                info[317] = 2
            buf = io.BytesIO()
            t0 = time.perf_counter()
            Image.fromarray(pixels).save(buf, format="TIFF", compression=pillow_name, tiffinfo=info)
            row["host_pillow_save"] = {"ms": round((time.perf_counter() - t0) * 1e3, 2), "bytes": len(buf.getvalue())}
            if compression == 5 and strips(file) != strips(buf.getvalue()):
                raise SystemExit(f"{pname} {cname}: the strips are not libtiff's")
            key = f"{pname}_{cname}"
            result["cases"][key] = row
            print(json.dumps({key: row}), flush=True)
            del d_out
        del d_pixels
    dev.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
