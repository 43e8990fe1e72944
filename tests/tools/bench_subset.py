"""Times cvhip_surface_subset on a surface of config 5's size: --rows rows (default 2048^2 = 4.19 M) with three
cameras, points and track rows in device memory, for kept counts of 10^4, 10^6 and rows - 1.  Per count: the median and spread
of the whole call (rows, points and track rows out), of the selection alone (rows out only) and, by difference, of the two
gathers; the restatement's rows are compared once.  Per-kernel times are not taken here: run the script under
`rocprofv3 --kernel-trace --stats -- python tests/tools/bench_subset.py --repeat 3` and read the subset_*_kernel rows.
For context, not as a gate: one host thread's numpy.argpartition plus fancy indexing of points and track rows on the same keys
(the keys are not counted) - what a caller did before cvhip_surface_subset, without the two copies between device and host.

    python tests/tools/bench_subset.py [--rows 4194304] [--repeat 7] [--seed 7] [--no-numpy] [--out profiles/x.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ref_subset  # noqa: E402
from cybervision_amd import _lib, correlation  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048 * 2048)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    n, m_cams = args.rows, 3
    rng = np.random.default_rng(1)
    points = rng.standard_normal((n, 3))
    tracks = rng.integers(-1, 2048, size=(n, m_cams, 2), dtype=np.int32)
    dev = correlation.create_gpu_context()
    L = _lib.lib()
    dp = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    d_points, d_tracks = torch.from_numpy(points).cuda(), torch.from_numpy(tracks).cuda()
    d_rows = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_opoints, d_otracks = torch.zeros_like(d_points), torch.zeros_like(d_tracks)
    torch.cuda.synchronize()
    out_n = C.c_uint64(0)

    def timed(fn, repeat):
        fn()  # (warm-up: the first launch loads the code object)
        times = []
        for _ in range(repeat):
            t1 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t1) * 1e3)
        return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "runs": repeat}

    keys = ref_subset.keys(n, args.seed)
    result = {"rows": n, "cameras": m_cams, "seed": args.seed, "device": dev.name() if hasattr(dev, "name") else "", "kept": []}
    for m in (10_000, 1_000_000, n - 1):
        if not 0 < m < n:
            continue

        def whole():
            _lib.check(L.cvhip_surface_subset(dev.handle, n, m, args.seed, dp(d_points), dp(d_tracks), m_cams, dp(d_rows), dp(d_opoints),
                                              dp(d_otracks), C.byref(out_n)), "cvhip_surface_subset")

        def selection():
            _lib.check(L.cvhip_surface_subset(dev.handle, n, m, args.seed, None, None, 0, dp(d_rows), None, None, C.byref(out_n)),
                       "cvhip_surface_subset")

        print(f"kept {m}", file=sys.stderr, flush=True)
        row = {"max_points": m, "call": timed(whole, args.repeat), "selection": timed(selection, args.repeat)}
        row["gathers_median_ms"] = round(row["call"]["median_ms"] - row["selection"]["median_ms"], 4)
        whole()
        want = ref_subset.select_smallest(keys, m)
        got = d_rows[:m].cpu().numpy().view(np.uint64)
        row["same_rows"] = bool(out_n.value == m and np.array_equal(got, want))
        row["same_points"] = bool(np.array_equal(d_opoints[:m].cpu().numpy(), points[want.astype(np.int64)]))
        if not args.no_numpy:
            def host():
                kept = np.sort(np.argpartition(keys, m - 1)[:m])
                return points[kept], tracks[kept]

            row["numpy_argpartition"] = timed(host, max(1, args.repeat // 3))
        result["kept"].append(row)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
