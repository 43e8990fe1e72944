"""The mixed rig that the multi-view tests share: a calibration matrix per camera, all different - fx != fy, skew of
either sign, a principal point off the centre by a different number of pixels in x and in y -, images of which no two
have the same (width, height), landscape and portrait mixed, and the true fundamental matrix of a pair whose two
cameras have different K.  Under one shared K with fx = fy, cx = cy, no skew and square images of one size, an
exchanged K1 / K2, an exchanged fx / fy or cx / cy, K[1] read for K[3], camera 0's K used for camera j and a transposed
(width, height) all compute the same numbers; here each of them changes the result (tests/test_triangulation_ref.py,
tests/test_pose_ref.py, tests/test_mesh_ref.py and tests/test_mesh_exact_ref.py show it on the CPU).

tri_scenes, pose_scenes and mesh_scenes build their mixed scenes from this module; it imports none of them."""
from __future__ import annotations

import numpy as np

# (width, height) of camera j: no two alike, four landscape, three portrait, one square
DIMS = [(2048, 1280), (1280, 2048), (1920, 1440), (1024, 1536), (2048, 2048), (1600, 900), (900, 1600), (1280, 1024)]


def dims(m, divisor=1):
    """The first m of DIMS, divided by `divisor` (4: the 225 .. 512 pixels of the pose scenes; 6.4: the 320 pixels on the
    long side of the mesh scenes), rounded to integers."""
    return [(int(round(w / divisor)), int(round(h / divisor))) for w, h in DIMS[:m]]


def calibration(j, size):
    """K of camera j with an image of size (w, h): fx = (0.45 + 0.07 j) w, fy = 1.25 fx (j odd) or 0.8 fx (j even), skew
    +-1.5 % of fx (negative for j odd), principal point (w / 2 + 17 - 5 j, h / 2 - 23 + 7 j) - off the centre by 17 - 5 j
    and -23 + 7 j pixels, which differ in size for every j and are never both 0."""
    w, h = size
    fx = (0.45 + 0.07 * j) * w
    fy = fx * (1.25 if j % 2 else 0.8)
    skew = (-0.015 if j % 2 else 0.015) * fx
    return np.array([[fx, skew, w / 2.0 + 17.0 - 5.0 * j], [0.0, fy, h / 2.0 - 23.0 + 7.0 * j], [0.0, 0.0, 1.0]])


def calibrations(sizes):
    return [calibration(j, s) for j, s in enumerate(sizes)]


def true_f(k1, k2, pose1, pose2):
    """F with x2^T F x1 = 0 for cameras K1 [R1 | t1] and K2 [R2 | t2]: K2^-T [t]x R K1^-1 with R = R2 R1^T and
    t = t2 - R t1, normalised by F[2][2] like the reference's models (synth.sfm_true_f, with two K)."""
    (r1, t1), (r2, t2) = pose1, pose2
    R = r2 @ r1.T
    t = t2 - R @ t1
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    F = np.linalg.inv(k2).T @ tx @ R @ np.linalg.inv(k1)
    return F / F[2, 2]


def common_view(Ks, boxes, margin):
    """The box of normalised image coordinates (x / z, y / z) that every camera K_j [I | 0] projects into
    [0, boxes[j][0]) x [0, boxes[j][1]), shrunk by `margin` on every side (for the cameras' small displacements)
    -> (x_lo, x_hi, y_lo, y_hi)."""
    y_lo = max((0.0 - K[1, 2]) / K[1, 1] for K in Ks) + margin
    y_hi = min((b[1] - 1.0 - K[1, 2]) / K[1, 1] for K, b in zip(Ks, boxes)) - margin
    reach = max(abs(y_lo), abs(y_hi))
    x_lo = max((0.0 - K[0, 2] + abs(K[0, 1]) * reach) / K[0, 0] for K in Ks) + margin
    x_hi = min((b[0] - 1.0 - K[0, 2] - abs(K[0, 1]) * reach) / K[0, 0] for K, b in zip(Ks, boxes)) - margin
    assert x_lo < x_hi and y_lo < y_hi
    return x_lo, x_hi, y_lo, y_hi
