"""Replay of the device RANSAC loops (cvhip_ransac_affine, cvhip_ransac_perspective) from their separately pinned
parts: the host restatement of the sampler (ref_ransac_sampler), the per-sample generators (the *_models hooks), the
exact fold (cvhip_ransac_score) and Ord's maximum (fundamentalmatrix.rs:623-649) carried in iteration order
(round, sample, root) with the reference's early exit (:135-141).  What the loops return must have these bits."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import ref_ransac_sampler as rs
from cybervision_amd import fundamentalmatrix as fm

ROUNDS = 20  # RANSAC_K / RANSAC_CHECK_INTERVAL


@dataclass
class Model:
    name: str
    n: int            # RANSAC_N
    tries: int
    min_count: int    # RANSAC_D + RANSAC_N
    exit_above: int   # RANSAC_RANK_EARLY_EXIT..: the loop ends after a round whose best count exceeds it

    def models(self, device, m, idx, t):
        if self.n == 4:
            return fm.affine_models_device(device, m, idx, t).reshape(len(idx), 1, 9)
        return fm.perspective_models_device(device, m, idx, t).reshape(len(idx), 3, 9)


AFFINE = Model("affine", 4, rs.TRIES_AFFINE, 14, 1000)
PERSPECTIVE = Model("perspective", 7, rs.TRIES_PERSPECTIVE, 207, 50_000)


@dataclass
class Replay:
    F: np.ndarray | None = None        # the winner [3, 3] (None: no hypothesis reached min_count)
    count: int = 0
    mean_error: float = float("nan")
    maxima: list = field(default_factory=list)   # the distinct matrices equal to the winner under Ord, in iteration order
    rounds_run: int = 0
    filled: list = field(default_factory=list)   # per round: the share of samples the sampler filled
    live: list = field(default_factory=list)     # per round: hypotheses that left the generator
    tied: list = field(default_factory=list)     # per round: hypotheses at the round's maximal count
    history: list = field(default_factory=list)  # per round: (F or None, count, number of maxima) as carried after it

    def after(self, rounds):
        """The carried best after `rounds` rounds (of a replay without early exit): (F or None, count, number of maxima)."""
        return self.history[rounds - 1]


def _ord_key(count, mean):
    """Ord: more inliers, then a finite mean error before a non-finite one, then the smaller one."""
    return (int(count), np.isfinite(mean), -mean if np.isfinite(mean) else 0.0)


_draws = {}


def draw_round(m, limit, seed, r, per_round, model):
    """rs.draw, remembered: scenes are replayed for both pencils, and a cluster scene's round costs seconds."""
    key = (hash(m.tobytes()), len(m), limit, seed, r, per_round, model.n, model.tries)
    if key not in _draws:
        _draws[key] = rs.draw(m, limit, seed, r, per_round, model.n, model.tries)
    return _draws[key]


def replay(device, matches, model: Model, seed: int, rounds: int, t: float, limit: int | None = None,
           per_round: int = rs.PER_ROUND) -> Replay:
    m = np.ascontiguousarray(np.asarray(matches, dtype=np.uint32).reshape(-1, 4))
    N = len(m)
    limit = rs.limit_of(N) if limit is None else limit
    may_exit = model is AFFINE or N > model.exit_above
    out = Replay()
    best_key = None
    seen = set()
    for r in range(rounds):
        out.rounds_run = r + 1
        idx, filled = draw_round(m, limit, seed, r, per_round, model)
        out.filled.append(float(filled.mean()))
        sel = np.flatnonzero(filled)          # unfilled samples are dead
        F = np.zeros((0, 9))
        if len(sel):
            F = model.models(device, m, idx[sel], t).reshape(-1, 9)   # iteration order: (sample, root)
            F = F[~np.isnan(F[:, 0])]                                  # drop the dead slots
        out.live.append(len(F))
        out.tied.append(0)
        if len(F):
            cnt, err = fm.ransac_score(device, F, m, t)
            cnt = cnt.astype(np.int64)
            top = int(cnt.max())
            if top >= model.min_count:
                at = np.flatnonzero(cnt == top)
                out.tied[-1] = len(at)
                mean = err[at] / top
                fin = np.isfinite(mean)
                if fin.any():
                    lo = mean[fin].min()
                    equal = at[fin & (mean == lo)]
                else:
                    lo = float("nan")
                    equal = at
                key = _ord_key(top, lo)
                if best_key is None or key > best_key:   # a later hypothesis replaces the carried one only if strictly better
                    best_key = key
                    out.F, out.count, out.mean_error = F[equal[0]].reshape(3, 3).copy(), top, float(lo)
                    out.maxima, seen = [], set()
                if key == best_key:
                    for h in equal:
                        b = F[h].tobytes()
                        if b not in seen:
                            seen.add(b)
                            out.maxima.append(F[h].reshape(3, 3).copy())
        out.history.append((None if out.F is None else out.F.copy(), out.count, len(out.maxima)))
        if may_exit and out.count > model.exit_above:   # :135-141
            break
    return out


class Listener:
    """The reference's progress listener (fundamentalmatrix.rs:41-47)."""

    def __init__(self):
        self.status, self.matches = [], []

    def report_status(self, p):
        self.status.append(p)

    def report_matches(self, c):
        self.matches.append(c)


def same_bits(a, b):
    return (np.asarray(a, dtype=np.float64).reshape(9).view(np.uint64) == np.asarray(b, dtype=np.float64).reshape(9).view(np.uint64)).all()
