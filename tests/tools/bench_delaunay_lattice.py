"""Times cvhip_mesh_delaunay's lattice path on what an affine surface gives it: the integer pixels of a
size^2 image without a seeded 10 % of them, points and faces in device memory.  Per size the median and the spread of the call
with cvhip_mesh_delaunay_set_lattice on and the share of the stars that the lattice kernels finished; with the switch off -
every star on the exact host path, the only way before - at --off-size only (larger sizes take minutes on the host).  The
switch-on call is timed a second time at --lane-cells (the stars of the boundary visit about sqrt(k / 2) cells: past the default
of 1024 from about 1500^2 points on).

    python tests/tools/bench_delaunay_lattice.py [--sizes 512,2048,4096] [--off-size 512] [--repeat 5] [--lane-cells 16384] [--out profiles/delaunay_lattice_bench.json]
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

from cybervision_amd import _lib, correlation, mesh  # noqa: E402


def lattice_with_holes(size, seed, share=0.10):
    keep = np.flatnonzero(np.random.default_rng(seed).random(size * size) >= share)
    return np.ascontiguousarray(np.stack([(keep % size).astype(np.float64), (keep // size).astype(np.float64)], axis=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,2048,4096")
    ap.add_argument("--off-size", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--lane-cells", type=int, default=16384, help="a second lane_cells to time with the switch on (0: none)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "delaunay_lattice_bench.json"))
    args = ap.parse_args()
    import torch

    dev = correlation.create_gpu_context()
    L = _lib.lib()
    result = {"device": dev.name() if hasattr(dev, "name") else "", "lane_cells": mesh.DELAUNAY_LANE_CELLS_DEFAULT, "sizes": []}
    for size in (int(v) for v in args.sizes.split(",")):
        xy = lattice_with_holes(size, size)
        k = len(xy)
        d_xy = torch.from_numpy(xy).cuda()
        d_faces = torch.zeros((2 * k, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        n, st = C.c_uint64(0), np.zeros(len(mesh.DELAUNAY_STATS), dtype=np.uint64)

        def call():
            _lib.check(L.cvhip_mesh_delaunay(dev.handle, C.c_void_p(d_xy.data_ptr()), k, C.c_void_p(d_faces.data_ptr()), 2 * k,
                                             C.byref(n), C.c_void_p(st.ctypes.data)), "cvhip_mesh_delaunay")

        def timed(repeat):
            times = []
            for _ in range(repeat):
                t1 = time.perf_counter()
                call()
                times.append((time.perf_counter() - t1) * 1e3)
            return {"median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3),
                    "runs": repeat}

        print(f"size {size}: {k} points, lattice on", file=sys.stderr, flush=True)
        mesh.set_delaunay_lattice(dev, True)
        call()  # (warm-up: the first launch loads the code object)
        row = {"size": size, "points": k, "lattice_on": timed(args.repeat), "faces": int(n.value),
               "stats": dict(zip(mesh.DELAUNAY_STATS, (int(v) for v in st))), "lattice_stars": mesh.delaunay_lattice_stars(dev)}
        row["lattice_star_share"] = row["lattice_stars"] / max(k, 1)
        if args.lane_cells:  # (a boundary star's half-plane crosses the whole grid: about sqrt(k / 2) cells)
            mesh.set_delaunay_lane_cells(dev, args.lane_cells)
            row["lane_cells_%d" % args.lane_cells] = dict(timed(args.repeat), host_stars=int(st[3]), most_cells=int(st[5]),
                                                          lattice_stars=mesh.delaunay_lattice_stars(dev))
            mesh.set_delaunay_lane_cells(dev, mesh.DELAUNAY_LANE_CELLS_DEFAULT)
        if size == args.off_size:
            first = d_faces[:n.value].clone()
            print(f"size {size}: lattice off (every star on the host)", file=sys.stderr, flush=True)
            mesh.set_delaunay_lattice(dev, False)
            row["lattice_off"] = timed(max(1, min(3, args.repeat)))
            row["lattice_off_host_stars"] = int(st[3])
            row["same_faces"] = bool(n.value == len(first) and torch.equal(d_faces[:n.value], first))
        mesh.set_delaunay_lattice(dev, mesh.DELAUNAY_LATTICE_DEFAULT)
        result["sizes"].append(row)
        del d_xy, d_faces
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
