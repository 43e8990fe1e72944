"""merge_tracks on config 5 (3 perspective views): reconstruct_perspective with merge_tracks=True records the table before
each of its merges; each is then merged again, timed three ways - cvhip_merge_tracks with host tables (upload, kernels,
readback of rows and table), with device tensors (tables already in HBM), and the numpy closed form of tests/ref_merge.py -
and checked against it.  Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python scripts/merge_bench.py`.  Prints one JSON line.

    python scripts/merge_bench.py --size 2048 [--repeat 5] [--out profiles/r08_merge_bench.json]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def _ms(fn, repeat, sync):
    times = []
    for _ in range(repeat):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, {"min_ms": min(times), "median_ms": statistics.median(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import ref_merge
    from cybervision_amd import _lib, correlation, reconstruction, synth, triangulation

    views, K, _ = synth.make_sfm_views(args.size)
    steps = synth.optimal_scale_steps(args.size, args.size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    tables = []
    merge = triangulation.PerspectiveTriangulation.merge_tracks

    def recording(self, device, image_index):
        tables.append((image_index, self.image_shapes[image_index], self.tracks.copy()))
        return merge(self, device, image_index)

    triangulation.PerspectiveTriangulation.merge_tracks = recording
    dev = correlation.create_gpu_context(ordinal=0)
    try:
        run = reconstruction.reconstruct_perspective(dev, pyrs, K, bundle_adjustment=False, seed=args.seed, merge_tracks=True)
        triangulation.PerspectiveTriangulation.merge_tracks = merge
        L = _lib.lib()
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        merges = []
        for image, (w, h), table in tables:
            n, m = table.shape[:2]
            rows = np.zeros(n, dtype=np.uint64)
            out = np.empty_like(table)
            stats = np.zeros(4, dtype=np.uint64)
            out_n = C.c_uint64(0)

            def host():
                _lib.check(L.cvhip_merge_tracks(dev.handle, p(table), n, m, image, w, h, p(rows), p(out), C.byref(out_n),
                                                p(stats)), "cvhip_merge_tracks")
                return out_n.value

            d_table = torch.from_numpy(table.reshape(-1)).cuda()
            d_rows = torch.empty(n, dtype=torch.int64, device="cuda")
            d_out = torch.empty(table.size, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def device():
                _lib.check(L.cvhip_merge_tracks(dev.handle, C.c_void_p(d_table.data_ptr()), n, m, image, w, h,
                                                C.c_void_p(d_rows.data_ptr()), C.c_void_p(d_out.data_ptr()), C.byref(out_n),
                                                None), "cvhip_merge_tracks")
                return out_n.value

            k, t_host = _ms(host, args.repeat, dev.synchronize)
            kd, t_dev = _ms(device, args.repeat, dev.synchronize)
            (want, want_stats), t_np = _ms(lambda: ref_merge.merge_tracks(table, image, w, h), 2, lambda: None)
            equal = (k == kd == len(want) and np.array_equal(rows[:k].astype(np.int64), want)
                     and np.array_equal(d_rows[:k].cpu().numpy(), want) and np.array_equal(out[:k], table[want])
                     and tuple(int(v) for v in stats) == want_stats)
            merges.append({"image": image, "rows_in": int(n), "rows_out": int(k), "present": int(stats[0]),
                           "cells": int(stats[1]), "rejected": int(stats[2]), "empty_area": int(stats[3]),
                           "table_mb": table.nbytes / 1e6, "host_tables": t_host, "device_tensors": t_dev,
                           "numpy_closed_form": t_np, "equal_to_restatement": bool(equal)})
            del d_table, d_rows, d_out
    finally:
        dev.close()
    res = {"config": 5, "size": args.size, "repeat": args.repeat, "camera_order": run["camera_order"],
           "reconstruct_merge_ms": run["timings_ms"].get("merge"), "merges": merges}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
