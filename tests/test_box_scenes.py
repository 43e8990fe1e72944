"""CPU checks of the stepped-walk scenes (tests/box_scenes.py): from the oracle's own search ranges at the last level,
each scene has box-kernel waves that walk 65 steps - one more than the walk's 64-lane step table - along a line that
changes row over them, in workgroups the wide stepped plan admits.  The GPU tests (test_corr_gpu.py) rely on it."""
import pytest

import box_scenes


@pytest.mark.parametrize("name", sorted(box_scenes.SCENES))
def test_stepped_scene_claims(oracle, name):
    c = box_scenes.make_scene(name)
    ranges = box_scenes.oracle_last_ranges(oracle, c)
    found = []
    for direction, (r, lines) in enumerate(ranges):
        h2, w2 = (c["img2"] if direction == 0 else c["img1"]).shape
        waves = box_scenes.box_waves(r, lines, (w2, h2), 2)
        # every wave of the scene is of the orientation it was made for
        assert waves and all(wv["tr"] == c["transposed"] for wv in waves)
        over = box_scenes.table_overruns(waves)
        for wv in over:
            # each pixel's own interval is within the stepped limit (<= 64 candidates), only the wave's union is 65
            assert wv["longest"] <= box_scenes.TABLE and wv["steps"] == box_scenes.TABLE + 1
            assert wv["steps_row"]  # step 0's rows are not step 64's
        found += over
    assert len(found) >= 4, f"{name}: {len(found)} waves walk 65 steps"
