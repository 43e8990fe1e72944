"""cvhip_ctx_set_fused_finish: the last level's forward cross-check runs inside complete()'s expansion (finish_grid_kernel)
instead of as a pass of its own.  Every way of asking for the result must give the same bits with the switch on, with it
off, and from the CPU oracle: xy equal, corr bit-equal where xy >= 0 and NaN elsewhere.

Scenes (tests/finish_scenes.py): widths that are no multiple of 64, heights that are no multiple of 4, w1 != w2, and enough
for the filter to do - test_scenes_give_the_filter_work counts, on the unfiltered grids, the removed cells, the cells whose
centre probe fails but whose window scan finds support, and the 64-cell row segments with an odd number of failing probes.
`ragged_dims` as tests/cases.py makes it has 16 removed cells and no such segment, so it is used with an occluded strip and
a displaced patch added to its second image (`ragged_dims_occluded`).  One count cannot be had from searched grids at all:
no cell within 5 pixels of an image border ever holds a match or is matched (the 11 x 11 correlation window), so no
searched grid has a failing cell within 4 cells of a border or a scan window clipped by one.  test_border_cells_on_edited_planes supplies those
through the four-call API instead: it rewrites both unfiltered planes (cvhip_ctx_level_grid) between the search calls and
the filter calls, with matches in and onto all four borders, and checks the result against the numpy restatement of the
filter - which every scene first shows equal to the oracle's."""
import functools

import numpy as np
import pytest

import cases
import finish_scenes
from cybervision_amd import correlation, sharding

pytestmark = pytest.mark.gpu
FWD, REV = correlation.CorrelationDirection.Forward, correlation.CorrelationDirection.Reverse
NONE = 0xFFFFFFFF
NAN_BITS = 0x7FC00000


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_grid(got, want, what, corr=True):
    gxy, gc = got
    wxy, wc = want
    diff = np.nonzero((np.asarray(gxy) != wxy).any(axis=-1))
    assert diff[0].size == 0, f"{what}: {diff[0].size} cells differ, first at (y, x) = ({diff[0][0]}, {diff[1][0]}): " \
                              f"got {gxy[diff[0][0], diff[1][0]]} want {wxy[diff[0][0], diff[1][0]]}"
    if corr:
        valid = wxy[..., 0] >= 0
        assert (bits(gc)[valid] == bits(wc)[valid]).all(), f"{what}: scores differ"
        assert np.isnan(gc[~valid]).all(), f"{what}: a None cell's score is not NaN"


@functools.lru_cache(maxsize=None)
def scene(name):
    """The scene, its pyramids and everything the oracle says about it (computed once, never modified)."""
    from oracle import cvref

    cvref.build()
    c = finish_scenes.make_scene(name)
    p1, p2 = cases.pyramids(c)
    ufwd, urev, want, want_rev = finish_scenes.unfiltered_last_level(cvref, c)
    for a in (ufwd, urev, *want, *want_rev):
        a.setflags(write=False)
    return dict(c=c, p1=p1, p2=p2, ufwd=ufwd, urev=urev, want=want, want_rev=want_rev)


def context(dev, s, fused_finish):
    c = s["c"]
    h1, w1 = c["img1"].shape
    h2, w2 = c["img2"].shape
    pc = correlation.PointCorrelations(dev, (w1, h1), (w2, h2), c["F"], correlation.ProjectionMode(c["projection"]))
    pc.set_fused_finish(fused_finish)
    return pc


def levels(pc, s, fused=True, p1=None, p2=None):
    p1, p2 = p1 or s["p1"], p2 or s["p2"]
    steps = s["c"]["steps"]
    pc.first_pass = True
    for i in range(steps + 1):
        k = steps - i
        pc.correlate_images(p1[k], p2[k], 1.0 / float(1 << k), fused=fused)


def both_switches(dev, s, body):
    """body(pc) with the switch on and off -> the two results."""
    out = []
    for on in (True, False):
        pc = context(dev, s, on)
        try:
            out.append(body(pc))
        finally:
            pc.close()
    return out


def plane(dev, ptr, lw, lh, dtype=np.uint32):
    dev.synchronize()
    return sharding.alias_bytes(ptr, lw * lh * 4, True).cpu().numpy().view(dtype).reshape(lh, lw)


def pack(xy):
    return np.where(xy[..., 0] >= 0, (xy[..., 1].astype(np.uint32) << 16) | xy[..., 0].astype(np.uint32), np.uint32(NONE))


ALL = pytest.mark.parametrize("name", finish_scenes.SCENES)


@ALL
def test_scenes_give_the_filter_work(gpu_device, name):
    """The unfiltered grids of the four-call API are the oracle's, the numpy restatement of the filter gives the oracle's
    filtered grids in both directions, and the scene exercises the kernel's paths (see the module docstring for the
    border count)."""
    s = scene(name)
    c = s["c"]
    pc = context(gpu_device, s, True)
    try:
        steps = c["steps"]
        for i in range(steps):
            k = steps - i
            pc.correlate_images(s["p1"][k], s["p2"][k], 1.0 / float(1 << k), fused=False)
        pc.correlate_images_step(s["p1"][0], s["p2"][0], 1.0, FWD)
        pc.correlate_images_step(s["p2"][0], s["p1"][0], 1.0, REV)
        gf, gr = pc.level_grid(FWD), pc.level_grid(REV)
        ufwd = pc.unpack_cells(plane(gpu_device, gf["cells"], gf["lw"], gf["lh"]))
        urev = pc.unpack_cells(plane(gpu_device, gr["cells"], gr["lw"], gr["lh"]))
    finally:
        pc.close()
    assert (ufwd == s["ufwd"]).all() and (urev == s["urev"]).all(), "unfiltered grids differ from the oracle's"
    _, kept = finish_scenes.restate_filter(ufwd, urev)
    _, kept_rev = finish_scenes.restate_filter(urev, ufwd)
    assert (kept == (s["want"][0][..., 0] >= 0)).all() and (kept_rev == (s["want_rev"][0][..., 0] >= 0)).all()
    n = finish_scenes.census(ufwd, urev)
    print(name, n)
    assert n["removed"] >= 100, n
    assert n["rescued"] >= 20, n
    assert n["odd_segments"] >= 1, n


@ALL
def test_complete_to_device_tensors(gpu_device, name):
    import torch

    s = scene(name)
    h1, w1 = s["c"]["img1"].shape

    def body(pc):
        levels(pc, s)
        oxy = torch.full((h1, w1, 2), 12345, dtype=torch.int32, device="cuda")
        oc = torch.full((h1, w1), 3.0, dtype=torch.float32, device="cuda")
        pc.complete(out_xy=oxy, out_corr=oc)
        gpu_device.synchronize()
        return oxy.cpu().numpy(), oc.cpu().numpy()

    on, off = both_switches(gpu_device, s, body)
    assert_grid(on, s["want"], "fused finish, device tensors")
    assert_grid(off, s["want"], "separate filter, device tensors")
    assert (on[0] == off[0]).all() and (bits(on[1]) == bits(off[1])).all()


@ALL
def test_complete_packed(gpu_device, name):
    s = scene(name)

    def body(pc):
        levels(pc, s)
        return pc.complete_packed()

    on, off = both_switches(gpu_device, s, body)
    assert (on[0] == pack(s["want"][0])).all() and (off[0] == on[0]).all()
    assert_grid((correlation.PointCorrelations.unpack_cells(on[0]), on[1]), s["want"], "fused finish, packed cells")
    assert (bits(on[1]) == bits(off[1])).all()
    assert (bits(on[1])[on[0] == NONE] == NAN_BITS).all()


@ALL
def test_complete_to_pageable_host_arrays(gpu_device, name):
    s = scene(name)

    def body(pc):
        levels(pc, s)
        return pc.complete()

    on, off = both_switches(gpu_device, s, body)
    assert_grid(on, s["want"], "fused finish, host arrays")
    assert_grid(off, s["want"], "separate filter, host arrays")
    assert (bits(on[1]) == bits(off[1])).all()


@ALL
def test_complete_without_scores(gpu_device, name):
    s = scene(name)
    h1, w1 = s["c"]["img1"].shape

    def body(pc):
        levels(pc, s)
        xy = np.full((h1, w1, 2), 777, dtype=np.int32)
        pc.complete(out_xy=xy, out_corr=None)
        return xy, None

    on, off = both_switches(gpu_device, s, body)
    assert_grid(on, s["want"], "fused finish, out_corr=None", corr=False)
    assert_grid(off, s["want"], "separate filter, out_corr=None", corr=False)


@ALL
def test_complete_twice(gpu_device, name):
    s = scene(name)

    def body(pc):
        levels(pc, s)
        return pc.complete(), pc.complete(), pc.complete_packed()

    for first, second, packed in both_switches(gpu_device, s, body):
        assert_grid(first, s["want"], "first complete()")
        assert_grid(second, s["want"], "second complete()")
        assert (packed[0] == pack(s["want"][0])).all()


@ALL
def test_level_grid_before_complete_is_filtered(gpu_device, name):
    s = scene(name)

    def body(pc):
        levels(pc, s)
        g = pc.level_grid(FWD)
        cells = plane(gpu_device, g["cells"], g["lw"], g["lh"]).copy()
        return cells, pc.complete()

    on, off = both_switches(gpu_device, s, body)
    assert (on[0] == off[0]).all(), "the plane handed out under fused finish is not the filtered one"
    assert (on[0] == pack(s["want"][0])).all()
    assert_grid(on[1], s["want"], "complete() after level_grid")
    assert_grid(off[1], s["want"], "complete() after level_grid, separate filter")


@ALL
def test_plane_after_complete_is_filtered(gpu_device, name):
    """complete() leaves the context's forward plane filtered, as the separate filter does."""
    s = scene(name)

    def body(pc):
        levels(pc, s)
        pc.complete()
        g = pc.level_grid(FWD)
        return plane(gpu_device, g["cells"], g["lw"], g["lh"]).copy()

    on, off = both_switches(gpu_device, s, body)
    assert (on == pack(s["want"][0])).all() and (off == on).all()


@ALL
@pytest.mark.parametrize("reverse_first", [True, False])
def test_reverse_grid_around_forward(gpu_device, name, reverse_first):
    s = scene(name)

    def body(pc):
        levels(pc, s)
        if reverse_first:
            rev = pc.complete(REV)
            return pc.complete(FWD), rev
        fwd = pc.complete(FWD)
        return fwd, pc.complete(REV)

    on, off = both_switches(gpu_device, s, body)
    for fwd, rev in (on, off):
        assert_grid(fwd, s["want"], "forward grid")
        assert_grid(rev, s["want_rev"], "reverse grid", corr=False)  # (its scores are the reference's only under exact scores)
    assert (on[1][0] == off[1][0]).all()


@ALL
@pytest.mark.parametrize("fuse_calls", [False, True])
def test_four_call_sequence(gpu_device, name, fuse_calls):
    s = scene(name)

    def body(pc):
        pc.set_fuse_level_calls(fuse_calls)
        levels(pc, s, fused=False)
        return pc.complete()

    on, off = both_switches(gpu_device, s, body)
    assert_grid(on, s["want"], "four calls, fused finish")
    assert_grid(off, s["want"], "four calls, separate filter")
    assert (bits(on[1]) == bits(off[1])).all()


@ALL
def test_triangulate_affine_without_complete(gpu_device, name):
    from oracle import cvref

    s = scene(name)

    def body(pc):
        levels(pc, s)
        tri = pc.triangulate_affine()
        return tri, pc.complete()

    want_pts, want_p2 = cvref.triangulate_affine(s["want"][0])
    for (pts, p2), grid in both_switches(gpu_device, s, body):
        assert pts.shape == want_pts.shape and (pts.view(np.uint64) == want_pts.view(np.uint64)).all()
        assert (p2 == want_p2).all()
        assert_grid(grid, s["want"], "complete() after triangulate_affine")


@ALL
def test_result_bands_and_row_band_do_not_defer(gpu_device, name):
    s = scene(name)
    h1 = s["c"]["img1"].shape[0]

    def banded(pc):
        pc.set_result_bands(2)
        levels(pc, s)
        return pc.complete(), pc.result_bands()

    on, off = both_switches(gpu_device, s, banded)
    assert on[1] == off[1]
    assert_grid(on[0], s["want"], "result bands, fused finish")
    assert_grid(off[0], s["want"], "result bands, separate filter")

    def row_band(pc):
        if not pc.set_row_band(0, 2):
            return None
        levels(pc, s)
        return pc.complete()

    on, off = both_switches(gpu_device, s, row_band)
    assert (on is None) == (off is None)
    if on is not None:
        r0, r1 = sharding.shard_rows(h1, 0, 2)
        for got in (on, off):
            assert_grid((got[0][r0:r1], got[1][r0:r1]), (s["want"][0][r0:r1], s["want"][1][r0:r1]), "row band 0 / 2")
        assert (on[0][r0:r1] == off[0][r0:r1]).all()


@ALL
def test_second_pair_without_complete_between(gpu_device, name):
    s = scene(name)
    o1 = [np.ascontiguousarray(p[::-1, ::-1]) for p in s["p1"]]  # another pair of the same dims, never completed
    o2 = [np.ascontiguousarray(p[::-1, ::-1]) for p in s["p2"]]

    def body(pc):
        levels(pc, s, p1=o1, p2=o2)
        levels(pc, s)
        return pc.complete()

    on, off = both_switches(gpu_device, s, body)
    assert_grid(on, s["want"], "second pair, fused finish")
    assert_grid(off, s["want"], "second pair, separate filter")


@ALL
def test_kernel_times_keep_their_keys(gpu_device, name):
    s = scene(name)

    def body(pc):
        pc.set_profiling(1, False)
        levels(pc, s)
        got = pc.complete()
        return got, pc.get_kernel_times()

    (on, kt_on), (off, kt_off) = both_switches(gpu_device, s, body)
    assert_grid(on, s["want"], "profiled, fused finish")
    assert_grid(off, s["want"], "profiled, separate filter")
    assert set(kt_on) == set(kt_off) == set(correlation.PointCorrelations.KERNEL_CLASSES)
    assert kt_on["expand"]["launches"] == 1 and kt_off["expand"]["launches"] == 1
    # the forward filter of the last level is inside `expand`: `cross_check` holds the other levels
    assert kt_on["cross_check"]["launches"] == kt_off["cross_check"]["launches"] - 1 == s["c"]["steps"]


@pytest.mark.parametrize("name", ["clusters_192x136", "ragged_dims_occluded"])
def test_border_cells_on_edited_planes(gpu_device, name):
    """Matches in the four-cell border of the forward grid, onto the borders of the reverse grid (scan windows clipped at
    all four sides) and onto cells that point back from a neighbour only: written into both unfiltered planes between the
    search calls and the filter calls.  The filtered grids must be the numpy restatement's, switch on or off."""
    import torch

    s = scene(name)
    c = s["c"]
    h1, w1 = c["img1"].shape
    h2, w2 = c["img2"].shape
    rng = np.random.default_rng(2024)
    fwd, rev = s["ufwd"].copy(), s["urev"].copy()
    border = [(x, y) for y in range(h1) for x in range(w1) if min(x, y, w1 - 1 - x, h1 - 1 - y) < 4 and (x + 2 * y) % 5 == 0]
    for x, y in border:
        # the match: anywhere near the cell's own position scaled into the reverse grid, often right on its border
        mx = int(np.clip(x * (w2 - 1) // (w1 - 1) + rng.integers(-3, 4), 0, w2 - 1))
        my = int(np.clip(y * (h2 - 1) // (h1 - 1) + rng.integers(-3, 4), 0, h2 - 1))
        fwd[y, x] = (mx, my)
        kind = rng.integers(0, 4)  # (2, 3: nothing supports it)
        if kind == 0:  # consistent: the probe finds it
            rev[my, mx] = (x, y)
        elif kind == 1:  # supported from elsewhere in the window, by a match near (not at) the cell
            ox, oy = int(np.clip(mx + rng.integers(-4, 5), 0, w2 - 1)), int(np.clip(my + rng.integers(-4, 5), 0, h2 - 1))
            rev[oy, ox] = (int(np.clip(x + rng.integers(-4, 5), 0, w1 - 1)), int(np.clip(y + rng.integers(-4, 5), 0, h1 - 1)))
    n = finish_scenes.census(fwd, rev)
    print(name, n)
    assert n["removed"] >= 100 and n["rescued"] >= 20 and n["odd_segments"] >= 1, n
    assert n["top"] and n["bottom"] and n["left"] and n["right"], n
    _, kept = finish_scenes.restate_filter(fwd, rev)
    _, kept_rev = finish_scenes.restate_filter(rev, fwd)
    in_border = np.zeros((h1, w1), dtype=bool)
    in_border[tuple(np.array(border).T[::-1])] = True
    assert (in_border & kept).sum() >= 20 and (in_border & ~kept).sum() >= 20, "border cells must be both kept and removed"
    want_xy = np.where(kept[..., None], fwd, -1)
    want_rev = np.where(kept_rev[..., None], rev, -1)

    def body(pc):
        steps = c["steps"]
        for i in range(steps):
            k = steps - i
            pc.correlate_images(s["p1"][k], s["p2"][k], 1.0 / float(1 << k), fused=False)
        pc.correlate_images_step(s["p1"][0], s["p2"][0], 1.0, FWD)
        pc.correlate_images_step(s["p2"][0], s["p1"][0], 1.0, REV)
        gf, gr = pc.level_grid(FWD), pc.level_grid(REV)
        sc = plane(gpu_device, gf["scores"], w1, h1, np.float32).copy()
        sc[(fwd != s["ufwd"]).any(axis=-1)] = 0.25  # (cells the search left None have no score of their own)
        for ptr, arr in ((gf["cells"], pack(fwd)), (gr["cells"], pack(rev)), (gf["scores"], sc)):
            sharding.alias_bytes(ptr, arr.size * 4, True).copy_(torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda())
        torch.cuda.synchronize()
        pc.cross_check_filter(1.0, FWD)
        pc.cross_check_filter(1.0, REV)
        got = pc.complete(FWD)
        return got, pc.complete(REV), sc

    on, off = both_switches(gpu_device, s, body)
    for got, got_rev, sc in (on, off):
        assert_grid(got, (want_xy, sc), "edited planes, forward")
        assert_grid(got_rev, (want_rev, None), "edited planes, reverse", corr=False)
    assert (bits(on[0][1]) == bits(off[0][1])).all()
