"""The dense track table in device memory (cvhip_tracks, triangulation.DeviceTrackTable) against the host-table
path around the same device entries - PerspectiveTriangulation.add_image_pair_dense / merge_tracks on a numpy table, numpy
indexing for the gathers.  Every stage is integer: every comparison is equality of bytes."""
import ctypes as C

import numpy as np
import pytest

import cases
from cybervision_amd import _lib, correlation, synth, triangulation

pytestmark = pytest.mark.gpu

INVALID = -1  # CVHIP_ERR_INVALID
W, H = 240, 180
MARKER = (7777, 8888)  # a point no grid produces: a slot that holds it must survive the fill rule


def _correlate(device, img1, img2, f, projection):
    steps = synth.optimal_scale_steps(img1.shape[1], img1.shape[0])
    p1, p2 = synth.box_pyramid(img1, steps), synth.box_pyramid(img2, steps)
    pc = correlation.PointCorrelations(device, (img1.shape[1], img1.shape[0]), (img2.shape[1], img2.shape[0]), f,
                                       correlation.ProjectionMode(projection))
    for s in range(steps + 1):
        k = steps - s
        pc.correlate_images(p1[k], p2[k], 1.0 / float(1 << k))
    return pc


@pytest.fixture(scope="module")
def pc(gpu_device):
    """persp_240x180, correlated once: both paths run on this context (extend_tracks resets its scratch on each call)."""
    case = cases.make_case("persp_240x180")
    ctx = _correlate(gpu_device, case["img1"], case["img2"], case["F"], case["projection"])
    yield ctx
    ctx.close()


def _start_table(n, m, image1, image2, seed):
    """n rows: about half with slot image2 holding MARKER, some rows without an image-1 point, some with one outside the
    grid; the other slots random points or none."""
    rng = np.random.default_rng(seed)
    t = np.full((n, m, 2), -1, dtype=np.int32)
    for j in range(m):
        have = rng.random(n) < 0.6
        t[have, j, 0] = rng.integers(0, W, size=int(have.sum()))
        t[have, j, 1] = rng.integers(0, H, size=int(have.sum()))
    kind = rng.random(n)
    inside, outside = kind < 0.7, kind >= 0.85  # (between them: no image-1 point)
    t[:, image1] = -1
    t[inside, image1, 0] = rng.integers(0, W, size=int(inside.sum()))
    t[inside, image1, 1] = rng.integers(0, H, size=int(inside.sum()))
    t[outside, image1, 0] = rng.integers(W, W + 60, size=int(outside.sum()))
    t[outside, image1, 1] = rng.integers(0, H + 60, size=int(outside.sum()))
    marked = rng.random(n) < 0.5
    t[:, image2] = -1
    t[marked, image2] = MARKER
    return t


def _host_extend(table, m, image1, image2, pc):
    """The host-table path: add_image_pair_dense on a numpy copy -> (table, the three counts from the host path's arrays)."""
    tri = triangulation.PerspectiveTriangulation(m, [(W, H)] * m)
    tri.tracks = table.copy()
    tp2, new_p1, _ = pc.extend_tracks(table[:, image1], max(W, H))
    counts = {"matched": int((tp2[:, 0] >= 0).sum()) if len(table) else 0,
              "filled": int(((table[:, image2, 0] < 0) & (tp2[:, 0] >= 0)).sum()) if len(table) else 0,
              "appended": len(new_p1)}
    tri.add_image_pair_dense(image1, image2, pc)
    return tri.tracks, counts


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


EXTEND_CASES = [(n, m, pair) for n in (0, 1, 255, 256, 257) for m in (2, 3, 8)
                for pair in ([(0, 1)] if m == 2 else [(0, 1), (2, 0)])]


@pytest.mark.parametrize("n,m,pair", EXTEND_CASES)
def test_extend_equals_the_host_table_path(gpu_device, pc, n, m, pair):
    image1, image2 = pair
    start = _start_table(n, m, image1, image2, seed=1000 * n + 10 * m + image1)
    table = triangulation.DeviceTrackTable(gpu_device, m)
    try:
        table.assign(start)
        assert table.rows == n and table.m == m and _same(table.numpy(), start)
        got = table.extend(pc, image1, image2, max(W, H))
        want, counts = _host_extend(start, m, image1, image2, pc)
        print("extend", n, m, pair, got)
        assert got == counts
        assert counts["appended"] > 100 and (n < 255 or 0 < counts["filled"] < counts["matched"])
        assert _same(table.numpy(), want)
        if n:
            kept = start[:, image2, 0] == MARKER[0]
            assert kept.any() and (table.numpy()[:n][kept, image2] == MARKER).all()
        # another pair of columns on top: the appended rows take part like any others
        second = (image2, image1) if m == 2 else ((1, 2) if pair == (0, 1) else (0, 1))
        got2 = table.extend(pc, second[0], second[1], max(W, H))
        want2, counts2 = _host_extend(want, m, second[0], second[1], pc)
        print("second extend", second, got2)
        assert got2 == counts2 and counts2["matched"] > n
        assert _same(table.numpy(), want2)
    finally:
        table.close()


def test_growth_keeps_the_rows(gpu_device, pc):
    """reserve_rows = 0 and three extends in a row: the capacity grows at least twice, geometrically, and the rows equal the
    host path's after each."""
    table = triangulation.DeviceTrackTable(gpu_device, 3, reserve_rows=0)
    try:
        assert (table.rows, table.capacity, table.data_ptr) == (0, 0, 0)
        want = np.full((0, 3, 2), -1, dtype=np.int32)
        caps = [table.capacity]
        for image1, image2 in ((0, 1), (1, 2), (2, 0)):
            got = table.extend(pc, image1, image2, max(W, H))
            want, counts = _host_extend(want, 3, image1, image2, pc)
            assert got == counts and table.rows == len(want)
            assert _same(table.numpy(), want)
            caps.append(table.capacity)
            assert caps[-1] >= table.rows and caps[-1] >= caps[-2]
            assert caps[-1] == caps[-2] or caps[-1] >= 2 * caps[-2]  # never a growth by less than doubling
        print("capacities", caps, "rows", table.rows)
        assert sum(b > a for a, b in zip(caps, caps[1:])) >= 2
    finally:
        table.close()


def test_reserve_is_kept(gpu_device):
    table = triangulation.DeviceTrackTable(gpu_device, 2, reserve_rows=1000)
    try:
        assert table.capacity >= 1000 and table.rows == 0 and table.data_ptr != 0
        rows = np.arange(300 * 2 * 2, dtype=np.int32).reshape(300, 2, 2)
        table.assign(rows)
        assert table.capacity >= 1000 and _same(table.numpy(), rows)
        assert table.merge(0, 2048, 2048)["rows_in"] == 300 and table.capacity >= 1000
    finally:
        table.close()


def test_out_of_bounds_match_leaves_the_table_unchanged(gpu_device):
    """Image 2 wider than image 1 (image 1 is the right part of the scene, image 2 all of it): matches lie right of the
    image-1 grid, and a track that merges one makes extend_tracks return its "Index out of bounds" - from the host path's
    entry and from the table's, which must leave the table byte for byte as it was."""
    a, b, _ = synth.make_pair(W, H, seed=21)
    img1 = np.ascontiguousarray(a[:, 96:])
    ctx = _correlate(gpu_device, img1, b, synth.F_HORIZONTAL, 0)
    w1 = img1.shape[1]
    table = triangulation.DeviceTrackTable(gpu_device, 2)
    try:
        ys, xs = np.mgrid[0:H:3, 0:w1:3]
        start = np.full((xs.size, 2, 2), -1, dtype=np.int32)
        start[:, 0, 0], start[:, 0, 1] = xs.reshape(-1), ys.reshape(-1)
        start[::2, 1] = MARKER
        with pytest.raises(_lib.CvhipError, match="Index out of bounds") as host:
            ctx.extend_tracks(start[:, 0], max(W, H))
        assert host.value.code == INVALID
        table.assign(start)
        before = (table.rows, table.capacity)
        with pytest.raises(_lib.CvhipError, match="Index out of bounds") as dev:
            table.extend(ctx, 0, 1, max(W, H))
        assert dev.value.code == INVALID
        assert (table.rows, table.capacity) == before and _same(table.numpy(), start)
    finally:
        table.close()
        ctx.close()


def test_merge_equals_merge_tracks_on_the_downloaded_table(gpu_device, pc):
    m = 3
    table = triangulation.DeviceTrackTable(gpu_device, m)
    try:
        table.extend(pc, 0, 1, max(W, H))
        table.extend(pc, 1, 2, max(W, H))
        start = table.numpy()
        assert len(start) > 1000
        for image_index in range(m):
            table.assign(start)
            tri = triangulation.PerspectiveTriangulation(m, [(W, H)] * m)
            tri.tracks = start.copy()
            want = tri.merge_tracks(gpu_device, image_index)
            got = table.merge(image_index, W, H)
            print("merge", image_index, got)
            assert got == want and 0 < got["rows_out"] <= got["rows_in"]
            assert table.rows == len(tri.tracks) and _same(table.numpy(), tri.tracks)
        # a merge that fails (image_index >= m) leaves the table as it was
        with pytest.raises(_lib.CvhipError) as err:
            table.merge(m, W, H)
        assert err.value.code == INVALID and _same(table.numpy(), tri.tracks)
        # no row in image 0: the table becomes empty; an empty table stays empty
        none = start.copy()
        none[:, 0] = -1
        table.assign(none)
        got = table.merge(0, W, H)
        assert (got["rows_in"], got["rows_out"], got["present"], table.rows) == (len(none), 0, 0, 0)
        assert table.numpy().shape == (0, m, 2)
        got = table.merge(1, W, H)
        assert (got["rows_in"], got["rows_out"], table.rows) == (0, 0, 0)
    finally:
        table.close()
    empty = triangulation.DeviceTrackTable(gpu_device, m)  # (never held a row: no capacity)
    try:
        assert empty.merge(2, W, H)["rows_out"] == 0 and empty.rows == 0
    finally:
        empty.close()


def _random_rows(n, m, seed):
    return np.random.default_rng(seed).integers(-1, 4096, size=(n, m, 2), dtype=np.int32)


@pytest.mark.parametrize("n", [0, 257])
def test_select_columns_assign_read(gpu_device, n):
    m = 5
    rows = _random_rows(n, m, 3)
    table = triangulation.DeviceTrackTable(gpu_device, m)
    try:
        table.assign(rows)
        for cols in ([0], [3], [0, 1, 2, 3, 4], [1, 4], [0, 2, 3]):
            sel = table.select_columns(cols)
            try:
                assert (sel.rows, sel.m) == (n, len(cols)) and _same(sel.numpy(), rows[:, cols])
                assert n == 0 or sel.data_ptr != table.data_ptr
            finally:
                sel.close()
        assert _same(table.numpy(), rows)  # (the source is only read)
        for bad in ([], [1, 1], [2, 1], [0, 5], [0, 1, 2, 3, 4, 5]):
            with pytest.raises(_lib.CvhipError) as err:
                table.select_columns(bad)
            assert err.value.code == INVALID
        if n:
            assert _same(table.numpy(5, 100), rows[5:105]) and _same(table.numpy(n, 0), rows[n:])
            import torch

            dev_rows = torch.from_numpy(rows[::-1].copy()).cuda()
            table.assign(dev_rows)  # from device memory
            assert _same(table.numpy(), rows[::-1])
            out = np.full((10, m, 2), 99, dtype=np.int32)
            for first, count in ((n - 9, 10), (n + 1, 0), (0, n + 1)):
                rc = _lib.lib().cvhip_tracks_read(table.handle, first, count, C.c_void_p(out.ctypes.data))
                assert rc == INVALID and (out == 99).all()
            table.assign(rows[:7])  # fewer rows than the capacity: in place
            assert table.rows == 7 and _same(table.numpy(), rows[:7])
        else:
            assert _lib.lib().cvhip_tracks_read(table.handle, 0, 1, C.c_void_p(rows.ctypes.data)) == INVALID
    finally:
        table.close()


def test_gather_host_and_device_rows(gpu_device):
    import torch

    n, m = 257, 3
    rows = _random_rows(n, m, 8)
    order = np.random.default_rng(9).integers(0, n, size=n + 40).astype(np.uint64)  # random order, with repeats
    assert len(np.unique(order)) < len(order)
    table = triangulation.DeviceTrackTable(gpu_device, m)
    try:
        table.assign(rows)
        want = rows[order.astype(np.int64)]
        host_out = np.empty((len(order), m, 2), dtype=np.int32)
        assert _same(table.gather(order, out=host_out), want)                      # host rows -> host out
        assert _same(table.gather(order).cpu().numpy(), want)                      # host rows -> device out
        dev_order = torch.from_numpy(order.astype(np.int64)).cuda()
        assert _same(table.gather(dev_order).cpu().numpy(), want)                  # device rows -> device out
        assert _same(table.gather(dev_order, out=np.empty_like(host_out)), want)   # device rows -> host out
        assert table.gather(np.zeros(0, dtype=np.uint64)).shape == (0, m, 2)
        # a row >= n: INVALID, nothing written - to a host output and to a device output
        bad = order.copy()
        bad[len(bad) // 2] = n
        host_out[:] = 99
        with pytest.raises(_lib.CvhipError) as err:
            table.gather(bad, out=host_out)
        assert err.value.code == INVALID and (host_out == 99).all()
        dev_out = torch.full((len(bad), m, 2), 99, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(_lib.CvhipError) as err:
            table.gather(torch.from_numpy(bad.astype(np.int64)).cuda(), out=dev_out)
        assert err.value.code == INVALID and bool((dev_out == 99).all())
        table.assign(rows[:0])
        with pytest.raises(_lib.CvhipError):
            table.gather(np.zeros(1, dtype=np.uint64))  # an empty table has no row 0
    finally:
        table.close()


def test_argument_errors(gpu_device, pc):
    L = _lib.lib()
    table = triangulation.DeviceTrackTable(gpu_device, 3)
    side = triangulation.DeviceTrackTable(gpu_device.side_handle(0), 3)
    try:
        start = _random_rows(20, 3, 2) % 100
        table.assign(start)
        side.assign(start)
        for image1, image2 in ((1, 1), (0, 3), (3, 0), (7, 9)):
            with pytest.raises(_lib.CvhipError) as err:
                table.extend(pc, image1, image2, max(W, H))
            assert err.value.code == INVALID
        with pytest.raises(_lib.CvhipError, match="another device handle") as err:
            side.extend(pc, 0, 1, max(W, H))  # pc belongs to gpu_device, the table to its side handle
        assert err.value.code == INVALID
        assert _same(table.numpy(), start) and _same(side.numpy(), start)
        out = C.c_void_p()
        assert L.cvhip_tracks_create(None, 3, 0, C.byref(out)) == INVALID
        assert L.cvhip_tracks_create(gpu_device.handle, 3, 0, None) == INVALID
        assert L.cvhip_tracks_create(gpu_device.handle, 0, 0, C.byref(out)) == INVALID
        assert L.cvhip_tracks_create(gpu_device.handle, triangulation.MAX_CAMERAS + 1, 0, C.byref(out)) == -3  # UNSUPPORTED
        assert L.cvhip_tracks_info(None, None, None, None, None) == INVALID
        assert L.cvhip_tracks_assign(None, None, 0) == INVALID
        assert L.cvhip_tracks_assign(table.handle, None, 1) == INVALID
        assert L.cvhip_tracks_read(None, 0, 0, None) == INVALID
        assert L.cvhip_tracks_read(table.handle, 0, 1, None) == INVALID
        assert L.cvhip_tracks_extend(None, pc._h, 0, 1, W, None) == INVALID
        assert L.cvhip_tracks_extend(table.handle, None, 0, 1, W, None) == INVALID
        assert L.cvhip_tracks_merge(None, 0, W, H, None) == INVALID
        assert L.cvhip_tracks_select_columns(None, None, 1, C.byref(out)) == INVALID
        assert L.cvhip_tracks_select_columns(table.handle, None, 1, C.byref(out)) == INVALID
        assert L.cvhip_tracks_gather(None, None, 0, None) == INVALID
        assert L.cvhip_tracks_gather(table.handle, None, 1, None) == INVALID
        L.cvhip_tracks_destroy(None)
        assert _same(table.numpy(), start)
    finally:
        table.close()
        side.close()


def test_uncorrelated_context_appends_nothing(gpu_device):
    ctx = correlation.PointCorrelations(gpu_device, (W, H), (W, H), cases.perspective_f(W, H), correlation.ProjectionMode(1))
    table = triangulation.DeviceTrackTable(gpu_device, 2)
    try:
        start = _start_table(40, 2, 0, 1, seed=5)
        table.assign(start)
        assert table.extend(ctx, 0, 1, max(W, H)) == {"matched": 0, "filled": 0, "appended": 0}
        assert _same(table.numpy(), start)
    finally:
        table.close()
        ctx.close()
