"""The dense track table in device memory through the C++ host layer (cybervision_amd/csrc/host/cvhip_host.hpp,
mesh::TrackTable) on a real GPU: a g++-built program correlates a small pair, then assign -> extend -> merge -> gather; every
table it writes must equal the ctypes path (triangulation.DeviceTrackTable) byte for byte."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cases
from cybervision_amd import correlation, synth, triangulation

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_host_tracks(gpu_device, tmp_path):
    exe = tmp_path / "host_tracks"
    lib_dir = ROOT / "cybervision_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "cpp" / "host_tracks.cpp"),
                           f"-L{lib_dir}", "-lcvhip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    case = cases.make_case("persp_240x180")
    h, w = case["img1"].shape
    m = 3
    rng = np.random.default_rng(6)
    start = np.full((300, m, 2), -1, dtype=np.int32)
    seen = rng.random(300) < 0.8
    start[seen, 0, 0], start[seen, 0, 1] = rng.integers(0, w, size=int(seen.sum())), rng.integers(0, h, size=int(seen.sum()))
    start[::3, 1] = (5, 6)
    start[:, 2, 0], start[:, 2, 1] = rng.integers(0, w, size=300), rng.integers(0, h, size=300)
    case["img1"].tofile(tmp_path / "img1.raw")
    case["img2"].tofile(tmp_path / "img2.raw")
    case["F"].tofile(tmp_path / "f.bin")
    start.tofile(tmp_path / "start.bin")
    res = subprocess.run([str(exe), str(tmp_path), str(w), str(h), str(m)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])

    steps = synth.optimal_scale_steps(w, h)
    p1, p2 = cases.pyramids(case)
    pc = correlation.PointCorrelations(gpu_device, (w, h), (w, h), case["F"], correlation.ProjectionMode(1))
    table = triangulation.DeviceTrackTable(gpu_device, m)
    try:
        for s in range(steps + 1):
            k = steps - s
            pc.correlate_images(p1[k], p2[k], 1.0 / float(1 << k))
        table.assign(start)
        counts = table.extend(pc, 0, 1, max(w, h))
        extended = table.numpy()
        merged_info = table.merge(0, w, h)
        merged = table.numpy()
        rows = (np.arange(500, dtype=np.uint64) * 7919) % np.uint64(len(merged))
        gathered = table.gather(rows, out=np.empty((500, m, 2), dtype=np.int32))
    finally:
        table.close()
        pc.close()
    assert info == {"rows_start": 300, "matched": counts["matched"], "filled": counts["filled"], "appended": counts["appended"],
                    "rows_extended": len(extended), "present": merged_info["present"], "cells": merged_info["cells"],
                    "rejected": merged_info["rejected"], "empty_area": merged_info["empty_area"], "rows_merged": len(merged), "m": m}
    assert counts["appended"] > 1000 and 0 < counts["filled"] < counts["matched"] and len(merged) > 1000
    assert np.fromfile(tmp_path / "after_extend.bin", dtype=np.int32).tobytes() == extended.tobytes()
    assert np.fromfile(tmp_path / "after_merge.bin", dtype=np.int32).tobytes() == merged.tobytes()
    assert np.fromfile(tmp_path / "gathered.bin", dtype=np.int32).tobytes() == gathered.tobytes()
