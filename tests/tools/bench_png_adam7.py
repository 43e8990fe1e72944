"""Times cvhip_png_ext_decode at size^2 on bench_png_in.py's photo-like picture as four RGB files: an Adam7
file whose rows are left to zlib as they are (filter type None: every row is a row segment), an Adam7 file of Paeth rows
throughout (a row segment per pass: seven side by side), and the same two not interlaced through the same entry point (the
all-Paeth one is a single segment, the unfilter pass's worst case).  Per file and format the end-to-end time of the whole
call with `out` in device memory (host clock around the call: the entry synchronises), as median and spread over --repeat
runs after --warmup, with cvhip_png_ext_last_stats beside it; the RGB8 must equal Pillow's.  For scale, not a gate: one host
thread of Pillow decoding the same bytes.  Nothing is promised in advance.  --once: every file once, RGB8 only, in the
order above and nothing else on the device - for a kernel trace of the run, whose k-th png_unfilter_kernel is the k-th file's.

    python tests/tools/bench_png_adam7.py [--size 2048] [--repeat 7] [--warmup 2] [--once] [--out profiles/x.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import io
import json
import statistics
import struct
import sys
import time
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_png_in import photo  # noqa: E402
from cybervision_amd import _lib, correlation, image  # noqa: E402

X0, Y0 = (0, 4, 0, 2, 0, 1, 0), (0, 0, 4, 0, 2, 0, 1)
DX, DY = (8, 8, 4, 4, 2, 2, 1), (8, 8, 8, 4, 4, 2, 2)


def filtered_rows(pixels, paeth_rows):
    """[h, w, 3] uint8 -> the filtered bytes of the (reduced) image: Paeth on every row, or None on every row."""
    h, w, _ = pixels.shape
    if not paeth_rows:
        return np.concatenate([np.zeros((h, 1), dtype=np.uint8), pixels.reshape(h, w * 3)], axis=1).tobytes()
    x = pixels.astype(np.int64).reshape(h, w * 3)
    up = np.concatenate([np.zeros((1, w * 3), dtype=np.int64), x[:-1]])
    a = np.concatenate([np.zeros((h, 3), dtype=np.int64), x[:, :-3]], axis=1)
    c = np.concatenate([np.zeros((h, 3), dtype=np.int64), up[:, :-3]], axis=1)
    p = a + up - c
    pa, pb, pc = abs(p - a), abs(p - up), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
    return np.concatenate([np.full((h, 1), 4, dtype=np.uint8), ((x - paeth) & 255).astype(np.uint8)], axis=1).tobytes()


def png_file(pixels, interlaced, paeth_rows):
    h, w, _ = pixels.shape
    if interlaced:
        parts = [pixels[Y0[p]::DY[p], X0[p]::DX[p]] for p in range(7)]
        filtered = b"".join(filtered_rows(part, paeth_rows) for part in parts if part.shape[0] and part.shape[1])
    else:
        filtered = filtered_rows(pixels, paeth_rows)

    def chunk(typ, body):
        return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, int(interlaced))) + chunk(b"IDAT", zlib.compress(filtered, 6)) +
            chunk(b"IEND", b""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.once:
        args.warmup, args.repeat = 0, 1
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
    files = {"adam7_none_rgb": png_file(pixels, True, False), "adam7_all_paeth_rgb": png_file(pixels, True, True),
             "plain_none_rgb": png_file(pixels, False, False), "plain_all_paeth_rgb": png_file(pixels, False, True)}
    result = {"size": args.size, "repeat": args.repeat, "warmup": args.warmup, "device": dev.name(), "files": {}}
    for name, data in files.items():
        file = np.frombuffer(data, dtype=np.uint8)
        row = {"file_bytes": len(data), "info": image.png_ext_info(data)}
        for mode, fmt, channels in (("rgb8", image.RGB8, 3), ("luma8", image.LUMA8, 1))[:1 if args.once else 2]:
            d_out = torch.empty(args.size * args.size * channels, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()  # (torch works on its own stream, the library on the handle's)

            def call():
                _lib.check(L.cvhip_png_ext_decode(dev.handle, C.c_void_p(file.ctypes.data), len(data), fmt, 0, C.c_void_p(d_out.data_ptr()), d_out.numel(),
                                                  C.byref(size_out)), "cvhip_png_ext_decode")

            row[mode] = {"device_out": timed(call), "stats": image.png_ext_last_stats()}
            row[mode]["device_out"]["pixel_gb_per_s"] = round(d_out.numel() / row[mode]["device_out"]["median_ms"] / 1e6, 2)
            got = d_out.cpu().numpy()
            t0 = time.perf_counter()
            im = Image.open(io.BytesIO(data))
            im.load()
            row[mode]["host_pillow_one_thread_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            if channels == 3 and not (im.mode == "RGB" and (got.reshape(args.size, args.size, 3) == np.asarray(im)).all()):
                raise SystemExit(f"{name}: the RGB8 is not Pillow's")
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
