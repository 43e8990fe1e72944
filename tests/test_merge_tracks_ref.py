"""The merge_tracks restatements against each other (no GPU): the literal transcription of the Rust folds and the numpy
closed form (tests/ref_merge.py)."""
import numpy as np
import pytest

import merge_scenes
import ref_merge


@pytest.mark.parametrize("x4, rows", [(25, [1, 4, 2]), (45, [4, 2])])
def test_worked_example(x4, rows):
    t = merge_scenes.worked_table(x4)
    w, h = merge_scenes.WORKED_SHAPE
    out_rows, stats = ref_merge.merge_tracks(t, 0, w, h)
    assert out_rows.tolist() == rows
    lit = ref_merge.merge_tracks_literal(t, 0, w, h)
    assert np.array_equal(lit, t[rows])
    # cell (3, 3) carries row 1's image-1 point (30, 3) when kept, not the mean (25, 3)
    if x4 == 25:
        assert lit[0, 1].tolist() == [30, 3]
    # 4 tracks seen in image 0, 3 occupied cells; (3, 4) and (6, 6) have an empty area cell
    assert stats == (4, 3, 3 - len(rows), 2)


def test_radius_and_distance():
    assert ref_merge.radius_and_distance(8, 8) == (2, 100)
    assert ref_merge.radius_and_distance(1000, 3) == (2, 100)
    assert ref_merge.radius_and_distance(3, 1001) == (2, 100)
    assert ref_merge.radius_and_distance(1500, 4) == (3, 150)
    assert ref_merge.radius_and_distance(2048, 2048) == (4, 204)
    assert ref_merge.radius_and_distance(4, 4100) == (8, 410)


def _agree(t, i, w, h):
    rows, stats = ref_merge.merge_tracks(t, i, w, h)
    lit = ref_merge.merge_tracks_literal(t, i, w, h)
    assert np.array_equal(lit, t[rows]), (t.shape, i, w, h)
    present = (t[:, i, 0] >= 0).sum() if len(t) else 0
    assert stats[0] == present and stats[1] - stats[2] == len(rows)
    return rows, stats


def test_random_small_tables_agree():
    rng = np.random.default_rng(11)
    rejected = kept = stacked = 0
    for case in range(300):
        w, h = int(rng.integers(1, 16)), int(rng.integers(1, 16))
        m = int(rng.integers(1, 5))
        i = int(rng.integers(0, m))
        n = int(rng.integers(0, 3 * w * h + 2))
        t = merge_scenes.random_table(rng, n, m, w, h, i, cells=int(rng.integers(1, w * h + 1)))
        rows, stats = _agree(t, i, w, h)
        rejected += stats[2]
        kept += len(rows)
        stacked += stats[0] > stats[1]
    # the cases reach both outcomes and cells with more than one track
    assert rejected > 50 and kept > 50 and stacked > 100


@pytest.mark.parametrize("w, h", [(1000, 3), (3, 1000), (1001, 4), (4, 1001), (1500, 3), (3, 1500), (4100, 2), (2, 4100)])
def test_radius_from_the_larger_side(w, h):
    rng = np.random.default_rng(w * 7 + h)
    for m in (2, 3):
        for i in range(m):
            t = merge_scenes.random_table(rng, 600, m, w, h, i, cells=300)
            _agree(t, i, w, h)


@pytest.mark.parametrize("dx, dy, kept", [(10, 0, True), (6, 8, True), (10, 1, False), (0, 11, False)])
def test_distance_at_the_bound(dx, dy, kept):
    """d^2 = 100 (md <= 1000): a distance of exactly d^2 merges, d^2 + 1 does not."""
    t = np.full((2, 2, 2), -1, dtype=np.int32)
    t[0] = [(2, 2), (50, 50)]
    t[1] = [(2, 3), (50 + dx, 50 + dy)]   # the area track of cell (2, 2) is row 1 (cell (2, 3) = (x*, yhi - 1))
    rows, _ = _agree(t, 0, 6, 4)
    assert (0 in rows.tolist()) == kept and 1 in rows.tolist()


def test_rows_without_an_image_i_point_are_dropped():
    t = np.full((3, 3, 2), -1, dtype=np.int32)
    t[0, 1] = (4, 4)
    t[1, 2] = (1, 1)
    t[2] = [(1, 1), (4, 4), (-1, -1)]
    rows, stats = _agree(t, 0, 5, 5)
    assert rows.tolist() == [2] and stats == (1, 1, 0, 1)   # (A of cell (1, 1) is cell (1, 2): empty)
    rows, stats = _agree(t, 1, 5, 5)
    assert rows.tolist() == [2] and stats == (2, 1, 0, 0)   # (0 and 2 share cell (4, 4): the highest row, 2, stays)
    empty, stats = _agree(t[:0], 0, 5, 5)
    assert len(empty) == 0 and stats == (0, 0, 0, 0)
