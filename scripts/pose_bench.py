"""Pose recovery on config 5 (3 perspective views): the sparse stage, then recover_camera_poses end to end (initial pair,
then the third camera), with batches run and linked-track counts.  Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python scripts/pose_bench.py`.  Prints one JSON line.

    python scripts/pose_bench.py --size 2048 [--repeat 3]
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from cybervision_amd import correlation, reconstruction, synth, triangulation

    views, K, poses = synth.make_sfm_views(args.size)
    steps = synth.optimal_scale_steps(args.size, args.size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    dev = correlation.create_gpu_context(ordinal=0)
    try:
        pairs = reconstruction.reconstruct_pairs(dev, pyrs, dense=False, seed=args.seed)
        runs = []
        for _ in range(args.repeat):
            tri = triangulation.PerspectiveTriangulation(3, [(args.size, args.size)] * 3, bundle_adjustment=False,
                                                         calibration=[K] * 3)
            for (i, j), e in sorted(pairs["pairs"].items()):
                if e["f"] is not None:
                    tri.add_image_pair_sparse(dev, i, j, e["f"], e["inliers"])
            dev.synchronize()
            t0 = time.perf_counter()
            first = tri.recover_next_cameras(dev, seed=args.seed)
            dev.synchronize()
            t1 = time.perf_counter()
            second = tri.recover_next_cameras(dev, seed=args.seed + 1)
            dev.synchronize()
            t2 = time.perf_counter()
            runs.append({"initial_pair": first, "initial_ms": (t1 - t0) * 1e3, "third": second, "third_ms": (t2 - t1) * 1e3,
                         **tri.last_pose, "tracks": int(len(tri.tracks))})
    finally:
        dev.close()
    best = min(runs, key=lambda r: r["initial_ms"] + r["third_ms"])
    print(json.dumps({"config": 5, "size": args.size, "recover_camera_poses_ms": best["initial_ms"] + best["third_ms"],
                      **best, "runs": len(runs)}))


if __name__ == "__main__":
    main()
