"""CPU checks of the lean box walk's fold (tests/fold_scenes.py): the schedule rule on random waves, by brute force, and
what the GPU scenes (test_box_fold_gpu.py) claim about themselves, from the oracle's own search ranges."""
import numpy as np
import pytest

import fold_scenes as fs


@pytest.mark.parametrize("shape", fs.SHAPES)
def test_schedule_rule_on_random_waves(shape):
    rng = np.random.default_rng(2024 + fs.SHAPES.index(shape))
    folded = {False: 0, True: 0}
    lengths = set()
    for _ in range(700):
        lo, hi, has = fs.random_wave(rng, shape)
        n = max(hi[l] for l in range(fs.LANES) if has[l]) + 1
        lengths.add(n)
        K, desc, seams = fs.schedule(lo, hi, has)
        Kc, descc, sel, base = fs.schedule_closed(lo, hi, has)
        # the kernel's closed form is the rule: the same K, the same orientation
        assert (K, desc if K else False) == (Kc, descc if Kc else False)
        assert 0 <= K <= n // 2
        rounds = fs.lane_steps(n, Kc, sel, base)
        assert len(rounds) == n - K
        fs.check_walk(lo, hi, has, rounds)
        # the lanes' sides are the rule's: one seam per pair, the lower side up to it
        for r, k in zip(rounds[n - 2 * K:], range(K - 1, -1, -1)):
            low_side = [l for l in range(fs.LANES) if r[l] == k]
            high_side = [l for l in range(fs.LANES) if r[l] == n - K + k]
            assert len(low_side) + len(high_side) == fs.LANES
            if low_side and high_side:
                assert (max(high_side) < min(low_side)) if desc else (max(low_side) < min(high_side))
            # any seam the rule admits separates the lanes that search: they sit on their own side with their windows
            s = seams[k]
            for l in range(fs.LANES):
                if has[l] and lo[l] <= k <= hi[l]:
                    assert (l - 10 > s) if desc else (l <= s)
                if has[l] and lo[l] <= n - K + k <= hi[l]:
                    assert (l <= s) if desc else (l - 10 > s)
        # K = 0 (the switch off) is the plain walk
        assert fs.lane_steps(n, Kc, sel, base, fold=False) == fs.plain_walk(n)
        fs.check_walk(lo, hi, has, fs.plain_walk(n))
        if K:
            folded[desc] += 1
    assert {1, 2, fs.MAX_STEPS - 1, fs.MAX_STEPS} <= lengths
    if shape in ("rising", "tent", "valley", "edge"):
        assert folded[False] >= 20
    if shape in ("falling", "tent", "valley", "edge"):
        assert folded[True] >= 20


def test_a_wave_that_every_lane_fills_does_not_fold():
    has = [l >= fs.LANE0 for l in range(fs.LANES)]
    lo, hi = [0] * fs.LANES, [16] * fs.LANES
    assert fs.schedule(lo, hi, has)[0] == 0 and fs.schedule_closed(lo, hi, has)[0] == 0
    # one lane alone folds nothing either: its interval is the union
    one = [l == 40 for l in range(fs.LANES)]
    assert fs.schedule_closed(lo, hi, one)[0] == 0


# scene -> (ascending, descending): at least a few dozen waves fold that way / none does
EXPECT = {
    "ramp_up": (True, None), "ramp_down": (None, True), "flat": (False, False), "tent_valley": (True, True),
    "edge": (True, True), "ramp_half": (None, None), "ramp_strip": (None, None),
}


@pytest.mark.parametrize("name", sorted(fs.SCENES))
def test_scene_claims(oracle, name):
    c = fs.make_scene(name)
    assert c["img1"].shape[1] <= 512 and c["img1"].shape[0] <= 128
    f = fs.scene_folds(oracle, c)
    asc, desc = EXPECT[name]
    assert f["waves"] > 0 and f["union"] - f["folded"] == f["asc"] + f["desc"]
    for want, waves in ((asc, f["waves_asc"]), (desc, f["waves_desc"])):
        if want is True:
            assert waves >= 36, f"{name}: {f}"
        elif want is False:
            assert waves == 0, f"{name}: {f}"
    if name == "ramp_half":
        # unions up to the walk's admission limit (65 steps per workgroup) and past it: such tiles decline
        lengths = [wv["n"] for direction, (r, lines) in enumerate(fs.last_ranges(oracle, c))
                   for wv in fs.lane_waves(r, lines, (c["img2"] if direction == 0 else c["img1"]).shape[::-1])]
        assert sum(1 for n in lengths if 56 <= n <= fs.MAX_STEPS) >= 36 and sum(1 for n in lengths if n > fs.MAX_STEPS) >= 36
    if name == "ramp_strip":
        # lanes without a pixel inside waves that fold
        holes = 0
        for direction, (r, lines) in enumerate(fs.last_ranges(oracle, c)):
            h2, w2 = (c["img2"] if direction == 0 else c["img1"]).shape
            for wv in fs.lane_waves(r, lines, (w2, h2)):
                inner = [l for l in range(fs.LANE0, fs.LANES) if wv["has"][l]]
                if fs.schedule_closed(wv["lo"], wv["hi"], wv["has"])[0] and any(not wv["has"][l] for l in range(inner[0], inner[-1])):
                    holes += 1
        assert holes >= 12, holes
        assert c["img1"].shape[1] % fs.S3_OUT == 7
