"""CPU check of what the scenes of tests/row_line_scenes.py claim about themselves (test_row_lines_gpu.py runs them), from
the oracle's own last-level lines: which passes have one line per image row, which rows have stripes that the binade rule
leaves open, and which rows' lines leave the image."""
import numpy as np
import pytest

import row_line_scenes as rs

# rows whose five stripes straddle a power of two when the line runs through the pixel's own row
BINADE_ROWS = [y for k in (4, 5, 6, 7, 8) for y in range((1 << k) - 2, (1 << k) + 2)]
_LINES = {}


def claims(oracle, name):
    key = rs.image_key(name)
    if key not in _LINES:
        c = rs.make_scene(name)
        _LINES[key] = [rs.row_claims(r, lines) for r, lines in rs.oracle_last_lines(oracle, c)]
    return _LINES[key]


@pytest.mark.parametrize("name", sorted(rs.SCENES))
def test_scene_claims(oracle, name):
    c = rs.make_scene(name)
    h1, w1 = c["img1"].shape
    assert max(c["img1"].shape + c["img2"].shape) <= 352 and c["steps"] == 2
    fwd, rev = claims(oracle, name)
    for d, cl in ((0, fwd), (1, rev)):
        assert len(cl["rows"]) >= 0.8 * (h1 - 2 * rs.KERNEL_SIZE), f"{name}: direction {d} searches {len(cl['rows'])} rows"
        if c["used"][d]:
            # the table's premise: row-major lines with slope +-0, one offset per row
            assert cl["row_major"] and cl["horizontal"] and cl["uniform"], f"{name} direction {d}: {cl['row_major']}, {cl['horizontal']}, {cl['uniform']}"
    F = c["F"]
    shift = float(F[2, 2] / F[1, 2]) if F[1, 2] != 0.0 else 0.0
    if c["used"] == (True, True):
        # lines `shift` rows above the pixel's row (forward) and below it (reverse): the open rows are the binade rows, moved
        for cl, s in ((fwd, shift), (rev, -shift)):
            want = [y for y in (int(b + s) for b in BINADE_ROWS) if y in cl["rows"]]
            assert sorted(cl["open"]) == sorted(set(want) | {y for y in cl["rows"] if y - s - rs.CORRIDOR <= 8.0})
            assert len(want) >= 16  # (four rows per binade, five binades; a shift of 12 moves those of row 16 above the searched rows)
        if name == "three_rows_off":
            assert all(fwd["rows"][y] == y - 3.0 for y in fwd["rows"]) and all(rev["rows"][y] == y + 3.0 for y in rev["rows"])
            assert fwd["outside"] == [y for y in sorted(fwd["rows"]) if y < 6] and rev["outside"] == []
        elif name == "leaves_at_top":
            # rows whose first stripes lie above the image: the casts of the reference saturate there and the kernel declines
            # (at least a workgroup's four rows; the rows above them have no match at the level before and are not searched)
            assert len([y for y in fwd["outside"] if fwd["rows"][y] - rs.CORRIDOR < 0.0]) >= 4 and rev["outside"] == []
        else:
            assert fwd["outside"] == [] and rev["outside"] == []
    if name == "f6_1e-12":
        assert fwd["row_major"] and fwd["horizontal"] and not fwd["uniform"]  # a lean launch whose lines move along the row
        assert not rev["horizontal"]
    if name == "f2_1e-12":
        assert rev["row_major"] and rev["horizontal"] and not rev["uniform"]
        assert not fwd["horizontal"]
    if name == "tilt3":
        assert not fwd["horizontal"] and not rev["horizontal"]
    if name == "vertical":
        assert not fwd["row_major"] and not rev["row_major"]
    if name == "wider_352x288":
        assert c["img2"].shape[1] != w1
