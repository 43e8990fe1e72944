"""Times the Deflate and tiled TIFF reader (cvhip_tiff_ext_decode) at size^2 with `out` in device memory:
bench_png_in.py's photo-like RGB picture as Deflate strips of about 8 KB, 64 KB and 1 MB and as one strip; the same picture in
256 x 256 Deflate tiles with Predictor 2; its first channel as an 8-bit grey LZW file in 256 x 256 tiles and in strips of the
same size.  Per file the end-to-end time of the whole call (host clock around it: the entry synchronises) as median and spread
over --repeat runs after --warmup, with cvhip_tiff_ext_last_stats; the pixels must equal the picture.  Yardsticks of the same
run, not gates: cvhip_png_decode on the picture as Pillow writes it (the one-stream inflate this generalises), cvhip_tiff_decode
on the LZW strip file, and one host thread of Pillow opening each file, timed with the same warm-up and repeats.

    python tests/tools/bench_tiff_ext.py [--size 2048] [--file all|NAME] [--repeat 7] [--warmup 2] [--out profiles/x.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
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
sys.path.insert(0, str(ROOT / "tests" / "tools"))

import tiff_ext_scenes  # noqa: E402
import tiff_scenes  # noqa: E402
from bench_png_in import photo  # noqa: E402
from cybervision_amd import _lib, correlation, image  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--file", default="all")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
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
    grey = np.ascontiguousarray(pixels[:, :, :1])
    row_bytes = args.size * 3
    z = lambda b: zlib.compress(b, 6)  # noqa: E731

    def strips(kb):
        return tiff_scenes.write(pixels, compression=8, rps=max(1, kb * 1024 // row_bytes), long_values=True, encoder=z)

    lzw_strips = []  # (the writer's LZW encoder is plain Python: the file is made once for both entry points)

    def grey_lzw_strips():
        if not lzw_strips:
            lzw_strips.append(tiff_scenes.write(grey, compression=5, rps=max(1, 65536 // args.size), long_values=True))
        return lzw_strips[0]

    png = io.BytesIO()
    Image.fromarray(pixels).save(png, format="PNG")
    files = (("rgb_deflate_strips_8k", lambda: strips(8), "cvhip_tiff_ext_decode", pixels),
             ("rgb_deflate_strips_64k", lambda: strips(64), "cvhip_tiff_ext_decode", pixels),
             ("rgb_deflate_strips_1m", lambda: strips(1024), "cvhip_tiff_ext_decode", pixels),
             ("rgb_deflate_one_strip", lambda: strips(1 << 30), "cvhip_tiff_ext_decode", pixels),
             ("rgb_deflate_tiles_256_predictor", lambda: tiff_ext_scenes.write_tiles(pixels, 256, 256, compression=8, predictor=2, encoder=z),
              "cvhip_tiff_ext_decode", pixels),
             ("grey_lzw_tiles_256", lambda: tiff_ext_scenes.write_tiles(grey, 256, 256, compression=5), "cvhip_tiff_ext_decode", grey),
             ("grey_lzw_strips", grey_lzw_strips, "cvhip_tiff_ext_decode", grey),
             ("yardstick_grey_lzw_strips_tiff_decode", grey_lzw_strips, "cvhip_tiff_decode", grey),
             ("yardstick_rgb_png_decode", png.getvalue, "cvhip_png_decode", pixels))
    result = {"size": args.size, "repeat": args.repeat, "warmup": args.warmup, "device": dev.name(), "files": {}}
    for name, make, entry, want in files:
        if args.file not in ("all", name):
            continue
        data = make()
        file = np.frombuffer(data, dtype=np.uint8)
        fmt = image.RGB8 if want.shape[2] == 3 else image.LUMA8
        d_out = torch.empty(want.size, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (torch works on its own stream, the library on the handle's)

        def call():
            _lib.check(getattr(L, entry)(dev.handle, C.c_void_p(file.ctypes.data), len(data), fmt, 0, C.c_void_p(d_out.data_ptr()), d_out.numel(),
                                         C.byref(size_out)), entry)

        row = {"file_bytes": len(data), "entry": entry, "device_out": timed(call)}
        row["device_out"]["pixel_gb_per_s"] = round(d_out.numel() / row["device_out"]["median_ms"] / 1e6, 2)
        row["stats"] = image.tiff_ext_last_stats() if entry == "cvhip_tiff_ext_decode" else image.tiff_last_stats() if entry == "cvhip_tiff_decode" else image.png_last_stats()
        if not (d_out.cpu().numpy().reshape(want.shape) == want).all():
            raise SystemExit(f"{name}: the pixels are not the picture's")
        row["host_pillow_one_thread"] = timed(lambda: np.asarray(Image.open(io.BytesIO(data))))
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
