#!/usr/bin/env python3
"""Writes tests/golden/orb_edges.npz: the CPU oracle's keypoints and descriptors of four scenes of tests/orb_edge_scenes.py
(stretch_scene(170), dim_scene(4), the 97 x 203 ragged image, the 128 x 160 periodic crop) and its match_points output for
the crop's keypoints against the ragged image's at thresholds 32 and 64.  CPU only; recorded results only.

    python tests/tools/gen_orb_golden.py

tests/test_orb_edges_ref.py holds the oracle to the file, tests/test_orb_edges_gpu.py the device: a change that moves
oracle/cvref_orb.c and csrc/orb_kernels.hip together no longer stays green."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import orb_edge_scenes as scenes  # noqa: E402
from oracle import cvref  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "orb_edges.npz"


def main():
    cvref.build()
    entries = scenes.golden_entries(cvref.orb_extract, cvref.match_points)
    np.savez_compressed(GOLDEN, **entries)
    for k, v in entries.items():
        print(f"{k}: {v.dtype} {v.shape}")
    print(f"{GOLDEN.relative_to(ROOT)}: {GOLDEN.stat().st_size} bytes")


if __name__ == "__main__":
    main()
