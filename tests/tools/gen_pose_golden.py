#!/usr/bin/env python3
"""Writes tests/golden/pose_runs.json: ref_pose.recover_pose with the device's index stream on the runs of
pose_scenes.RANSAC_RUNS that take all 100 batches, too slow to restate in a test (stage_scrambled is the failing call
of the restated sparse stage on pose_scenes.scrambled_scene, so it needs the CPU oracle's extend_tracks).  CPU only;
the batches are independent (the carried result is folded in afterwards, in batch order), so they are spread over
worker processes, 16 at the most.

    python tests/tools/gen_pose_golden.py [--workers 16]

Per run: the scene parameters, the image, the seed, a digest of the track table, linked, ransac_d, count, error,
batches, winner, accepted, r, t, projection, the best (count, error, winner) after every batch, and for the scene claim
of tests/test_pose_ref.py the number of `contenders` (scored poses whose count is within 1 of the final one) and
`margin`, the smallest distance in pixels between a linked track's error and the threshold over all contenders.
tests/test_pose_ref.py re-derives batch 0 and the winner's batch."""
import argparse
import json
import sys
import time
from multiprocessing import Pool
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import pose_checks  # noqa: E402
import pose_scenes  # noqa: E402
import ref_pose as rp  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "pose_runs.json"
FIXTURE_RUNS = ("accepted_late", "scrambled_rejected", "stage_scrambled")


_CACHE = {}


def run_inputs(name):
    """-> (tracks, points, ok, projections, image, K, max_dimension, seed) of a run: the points are the restatement's."""
    if name not in _CACHE:
        _CACHE[name] = pose_checks.run_inputs(name)
    return _CACHE[name]


def batch_with_contenders(name, batch):
    """-> (recover_pose_batch's result, [(count, margin)] of its scored poses)."""
    tracks, pts, ok, projections, image, K, max_dimension, seed = run_inputs(name)
    lt, lp = rp.linked(tracks, pts, ok, image)
    thr = rp.RANSAC_T * max_dimension
    seen = []

    def observe(_batch, _h, _slot, count, _error, errs):
        with np.errstate(all="ignore"):
            seen.append((count, float(np.nanmin(np.abs(errs - thr)))))

    best = rp.recover_pose_batch(lt, lp, projections, image, K, max_dimension, seed, batch, observe=observe)
    return best, seen


def _work(job):
    return job, batch_with_contenders(*job)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=16)
    args = ap.parse_args()
    batches = rp.RANSAC_K // rp.RANSAC_CHECK_INTERVAL
    out = {"scene": {k: list(v) if isinstance(v, tuple) else v for k, v in pose_scenes.RANSAC_SCENE.items()}, "runs": {}}
    for name in FIXTURE_RUNS:
        t0 = time.time()
        with Pool(min(args.workers, 16)) as pool:
            done = dict(pool.imap_unordered(_work, [(name, b) for b in range(batches)]))
        tracks, pts, ok, projections, image, K, max_dimension, seed = run_inputs(name)
        res = rp.recover_pose(tracks, pts, ok, projections, image, K, max_dimension, seed,
                              batch_results={b: done[(name, b)][0] for b in range(batches)})
        near = [mg for b in range(res["batches"]) for c, mg in done[(name, b)][1] if c >= res["count"] - 1]
        r, t, P = res["best"]
        out["runs"][name] = {
            **pose_scenes.RANSAC_RUNS[name], "image": image, "seed": seed, "table": pose_checks.table_digest(tracks),
            "linked": res["linked"], "ransac_d": res["ransac_d"], "count": res["count"],
            "error": res["error"], "batches": res["batches"], "winner": list(res["winner"]),
            "accepted": res["camera"] is not None, "r": r.tolist(), "t": t.tolist(), "projection": P.tolist(),
            "history": [[c, e, list(w) if w else None] for c, e, w in res["history"]],
            "contenders": len(near), "margin": min(near), "cpu_seconds": round(time.time() - t0, 1),
            "workers": min(args.workers, 16)}
        print(name, {k: v for k, v in out["runs"][name].items() if k not in ("history", "projection")}, flush=True)
    GOLDEN.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
