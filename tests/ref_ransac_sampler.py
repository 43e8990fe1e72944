"""Host restatement of the sampler of the device RANSAC loops (ransac_generate_affine_kernel and
ransac_perspective_pencil_kernel in csrc/ransac_kernels.hip): choose_inliers (fundamentalmatrix.rs:155-175) on a
counter-based generator instead of the reference's OS-seeded one.

  state = mix64(seed ^ mix64(round << 32 | h))             per sample h of a round
  state = mix64(state + 0x9E3779B97F4A7C15)                per draw
  index = ((state >> 32) * limit) >> 32                    limit = min(N, 5000): only the head of the list is drawn from

A drawn match is taken unless one of its four coordinates lies within 10 pixels of the same coordinate of a match the
sample already holds; a sample that is not complete after `max_tries` draws (256 affine, 512 perspective) is given up
and produces no hypothesis.  numpy uint64 over the samples of a round, a plain loop over the tries."""
from __future__ import annotations

import numpy as np

TOP_INLIERS = 5000        # fundamentalmatrix.rs: choose_inliers draws from the first 5000 matches
MIN_PIXEL_DISTANCE = 10   # :160-170
TRIES_AFFINE, TRIES_PERSPECTIVE = 256, 512
PER_ROUND = 50_000        # RANSAC_CHECK_INTERVAL
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def mix64(z):
    """splitmix64's finaliser on uint64 (scalars or arrays; Python ints are taken modulo 2^64)."""
    if isinstance(z, int):
        z &= 0xFFFFFFFFFFFFFFFF
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def limit_of(n_matches):
    return min(int(n_matches), TOP_INLIERS)


def draw(matches, limit, seed, round, H, n, max_tries):
    """The samples h = 0 .. H-1 of round `round`: -> (idx [H, n] uint32, filled [H] bool).  Rows of idx that are not
    filled hold the matches taken before the sample was given up, then zeros."""
    m = np.asarray(matches).reshape(-1, 4).astype(np.int64)
    h = np.arange(H, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = (np.uint64(round) << np.uint64(32)) | h
        state = mix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ mix64(key))
        idx = np.zeros((H, n), dtype=np.uint32)
        have = np.zeros(H, dtype=np.int64)
        active = np.arange(H)
        slots = np.arange(n)
        # short lists (the cluster scenes, where nearly every draw is rejected): which pairs of matches are too close, once
        head = m[:limit]
        table = (np.abs(head[:, None, :] - head[None, :, :]) < MIN_PIXEL_DISTANCE).any(axis=2) if limit <= 2048 else None
        for _ in range(max_tries):
            if active.size == 0:
                break
            st = mix64(state[active] + GOLDEN)
            state[active] = st
            cand = ((st >> np.uint64(32)) * np.uint64(limit)) >> np.uint64(32)
            cand = cand.astype(np.int64)
            if table is not None:
                near = table[cand[:, None], idx[active]]                                                # [A, n]
            else:
                near = (np.abs(m[idx[active]] - m[cand][:, None, :]) < MIN_PIXEL_DISTANCE).any(axis=2)
            close = (near & (slots[None, :] < have[active][:, None])).any(axis=1)
            took = active[~close]
            idx[took, have[took]] = cand[~close]
            have[took] += 1
            active = active[have[active] < n]
    return idx, have == n
