"""Times the PNG decoder (cvhip_png_decode) on four files at size^2: a Pillow-written RGB file of a photo-like
picture (synth's value-noise texture per channel, rectangles and two bits of noise), the same picture written by
cvhip_png_encode, a 16-bit grey file of its first channel (Pillow), and the picture as a file of Paeth rows throughout (one
row segment: the unfilter pass's worst case).  Per file and format the end-to-end time of the whole call with `out` in device
memory (host clock around the call: the entry synchronises), as median and spread over --repeat runs after --warmup, with
cvhip_png_last_stats beside it; the RGB8 must equal Pillow's.  For scale, not a gate: one host thread of Pillow decoding the
same bytes.  Nothing is promised in advance.

    python tests/tools/bench_png_in.py [--size 2048] [--repeat 7] [--warmup 2] [--out profiles/x.json]
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

from cybervision_amd import _lib, correlation, image, mesh, synth  # noqa: E402


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


def all_paeth(pixels):
    """The RGB picture as a PNG file whose every row has filter type 4."""
    h, w, _ = pixels.shape
    x = pixels.astype(np.int64).reshape(h, w * 3)
    up = np.concatenate([np.zeros((1, w * 3), dtype=np.int64), x[:-1]])
    a = np.concatenate([np.zeros((h, 3), dtype=np.int64), x[:, :-3]], axis=1)
    c = np.concatenate([np.zeros((h, 3), dtype=np.int64), up[:, :-3]], axis=1)
    p = a + up - c
    pa, pb, pc = abs(p - a), abs(p - up), abs(p - c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
    rows = np.concatenate([np.full((h, 1), 4, dtype=np.uint8), ((x - pred) & 255).astype(np.uint8)], axis=1)

    def chunk(typ, body):
        return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) +
            chunk(b"IEND", b""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
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

    def pillow(array):
        buf = io.BytesIO()
        Image.fromarray(array).save(buf, "PNG")
        return buf.getvalue()

    pixels = photo(args.size)
    files = {"pillow_rgb": pillow(pixels), "own_encoder_rgb": mesh.png(dev, pixels).tobytes(), "pillow_grey16": pillow(pixels[:, :, 0].astype(np.uint16) * 257),
             "all_paeth_rgb": all_paeth(pixels)}
    result = {"size": args.size, "repeat": args.repeat, "warmup": args.warmup, "device": dev.name(), "files": {}}
    for name, data in files.items():
        file = np.frombuffer(data, dtype=np.uint8)
        row = {"file_bytes": len(data), "info": image.png_info(data)}
        for mode, fmt, channels in (("rgb8", image.RGB8, 3), ("luma8", image.LUMA8, 1)):
            d_out = torch.empty(args.size * args.size * channels, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()  # (torch works on its own stream, the library on the handle's)

            def call():
                _lib.check(L.cvhip_png_decode(dev.handle, C.c_void_p(file.ctypes.data), len(data), fmt, 0, C.c_void_p(d_out.data_ptr()), d_out.numel(),
                                              C.byref(size_out)), "cvhip_png_decode")

            row[mode] = {"device_out": timed(call), "stats": image.png_last_stats()}
            row[mode]["device_out"]["pixel_gb_per_s"] = round(d_out.numel() / row[mode]["device_out"]["median_ms"] / 1e6, 2)
            got = d_out.cpu().numpy()
            t0 = time.perf_counter()
            im = Image.open(io.BytesIO(data))
            im.load()
            row[mode]["host_pillow_one_thread_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            if channels == 3 and im.mode == "RGB" and not (got.reshape(args.size, args.size, 3) == np.asarray(im)).all():
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
