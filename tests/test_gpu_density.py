"""GPU: the density measures, csrc/k_density_roi.hip against the numpy restatement (tests/_density_ref.py) under
``==`` -- cnt, s1, s2, lo, hi of every region -- at the sizes where the box is one lane, one wave and one workgroup (each +- 1),
on the three orientations, on views with negative strides, at int16's ends, in batches, at the polygon cap, bound and unbound,
on the resident volume; the ellipses equal the numbers the reference itself produced (tests/golden/ref_density.npz)."""
import ctypes
import gc
import os

import numpy as np
import pytest

import _density_ref as R

from invesalius3_amd.measures import density_of  # noqa: F401  (the feature under test: without it this file fails at import)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (16, 20, 24)  # dz, dy, dx: a 24 x 20 x 16 volume
SPACING = (0.5, 0.5, 2.0)


@pytest.fixture(autouse=True)
def _registry_returns_to_what_it_was(ivxlib):
    from invesalius3_amd import resident
    before = resident.count()
    yield
    resident.set_check(False)
    gc.collect()
    assert resident.count() == before


@pytest.fixture(scope="module")
def volume():
    rng = np.random.default_rng(7)
    v = rng.integers(-1024, 3072, SHAPE).astype(np.int16)
    v[8, 10, 12], v[8, 9, 12], v[7, 10, 12], v[8, 10, 11] = -32768, 32767, 32767, -32768
    v.setflags(write=False)
    return v


def want_record(M, image, spacing, m):
    """the restatement's record of one measure (None where the reference raises IndexError)"""
    grid_image = image if image.ndim == 3 else image[None]
    img = R.slice_of(grid_image, m.orientation, m.slice_number)
    h, w = img.shape
    if isinstance(m, M.CircleDensityMeasure):
        par = R.ellipse_params(m.orientation, spacing, m.center, m.point1, m.point2)
        return R.record(img[R.ellipse_mask(h, w, *par)])
    return R.record(img[R.polygon_mask(h, w, R.polygon_points(m.orientation, spacing, m.points))])


def records(M, image, spacing, measures):
    q, pts = M.describe_rois(M._Grid.of(image), spacing, measures)
    return M.roi_records(q, len(measures), pts)


def check(M, image, spacing, measures):
    got = records(M, image, spacing, measures)
    want = np.array([want_record(M, image, spacing, m) for m in measures], np.int64).reshape(-1, 5)
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    return got


def mixed_measures(M, n, shape=SHAPE, spacing=SPACING):
    """n measures that mix kinds, orientations and empty selections"""
    dz, dy, dx = shape
    ext = (dx * spacing[0], dy * spacing[1], dz * spacing[2])
    rng = np.random.default_rng(100 + n)
    out = []
    for k in range(n):
        ori = ("AXIAL", "CORONAL", "SAGITAL")[k % 3]
        sl = int(rng.integers(0, shape[k % 3]))
        c = tuple(rng.uniform(0, e) for e in ext)
        if k % 5 == 3:  # wholly outside: empty
            c = tuple(-3.0 * e - 5.0 for e in ext)
        if k % 2 == 0:
            ra, rb = rng.uniform(0.3, 6.0, 2)
            if k % 7 == 6:
                ra = 0.0  # a == 0: nothing
            i, j = R.PLANE[ori]
            p1, p2 = list(c), list(c)
            p1[i] += ra
            p2[j] -= rb
            out.append(M.CircleDensityMeasure(ori, sl, c, tuple(p1), tuple(p2)))
        else:
            npts = (0, 1, 2, 3, 4, 7, 12)[k % 7]
            pts = [tuple(np.array(c) + rng.uniform(-6, 6, 3)) for _ in range(npts)]
            out.append(M.PolygonDensityMeasure(ori, sl, pts))
    return out


# ---- 1. the box at one lane, one wave, one workgroup -----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (64, 4), (65, 63), (257, 3), (130, 130)])
def test_slice_shapes(ivxlib, shape):
    from invesalius3_amd import measures as M
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    img = rng.integers(-2000, 4000, shape).astype(np.int16)
    c = (w / 2.0, h / 2.0, 0.0)
    whole = M.CircleDensityMeasure("AXIAL", 0, c, (c[0] + 3.0 * w + 5, c[1], 0.0), (c[0], c[1] + 3.0 * h + 5, 0.0))
    inner = M.CircleDensityMeasure("AXIAL", 0, c, (c[0] + w / 3.0, c[1], 0.0), (c[0], c[1] - h / 2.5, 0.0))
    corner = M.CircleDensityMeasure("AXIAL", 0, (0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0))
    frame = M.PolygonDensityMeasure("AXIAL", 0, [(-1.0, -1.0, 0.0), (w + 1.0, -1.0, 0.0), (w + 1.0, h + 1.0, 0.0), (-1.0, h + 1.0, 0.0)])
    tri = M.PolygonDensityMeasure("AXIAL", 0, [(0.0, 0.0, 0.0), (w * 1.0, h * 0.5, 0.0), (w * 0.25, h * 1.0, 0.0)])
    got = check(M, img, (1.0, 1.0, 1.0), [whole, inner, corner, frame, tri])
    assert got[0, 0] == h * w == got[3, 0] and got[2, 0] >= 1


# ---- 2. orientations, int16's ends, strides ----------------------------------------------------------------------------------
def orientation_measures(M):
    out = []
    for ori, sl in (("AXIAL", 8), ("CORONAL", 10), ("SAGITAL", 12), ("AXIAL", 0), ("CORONAL", 19), ("SAGITAL", 23)):
        i, j = R.PLANE[ori]
        c = [6.0, 5.0, 16.0]  # mm: voxel (12, 10, 8), where the extremes sit
        p1, p2, e1, e2 = list(c), list(c), list(c), list(c)
        p1[i] += 2.5 * SPACING[i]
        p2[j] += 3.0 * SPACING[j]
        out.append(M.CircleDensityMeasure(ori, sl, tuple(c), tuple(p1), tuple(p2)))
        e1[i], e2[j] = -1.0, c[j] + 40.0  # cut by the slice's edges
        out.append(M.CircleDensityMeasure(ori, sl, (0.0, 0.0, 0.0), tuple(e1), tuple(e2)))
        pts = []
        for a, b in ((2.2, 1.1), (10.6, 3.0), (8.0, 9.1), (5.5, 5.0), (1.5, 8.7)):
            p = list(c)
            p[i], p[j] = a * SPACING[i], b * SPACING[j]
            pts.append(tuple(p))
        out.append(M.PolygonDensityMeasure(ori, sl, pts))
    return out


def test_three_orientations_and_the_ends_of_int16(ivxlib, volume):
    from invesalius3_amd import measures as M
    got = check(M, volume, SPACING, orientation_measures(M))
    assert got[0, 3] == -32768 and got[0, 4] == 32767 and (got[:9, 0] > 0).all()


@pytest.mark.parametrize("bound", [False, True])
def test_views_with_negative_and_odd_strides(ivxlib, volume, bound):
    from invesalius3_amd import measures as M
    from invesalius3_amd import resident
    parent = np.array(volume)
    r = resident.bind(parent) if bound else None
    try:
        for view in (parent[:, ::-1, :], parent[::-1], parent[:, :, ::-1], parent[::-1, ::-1, ::-1], parent[:, 1:, 1:], parent[::2, :, ::3]):
            ms = mixed_measures(M, 9, view.shape)
            check(M, view, SPACING, ms)
    finally:
        if r is not None:
            r.release()


# ---- 3. batches ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 65])
def test_batches_equal_one_by_one(ivxlib, volume, n):
    from invesalius3_amd import measures as M
    ms = mixed_measures(M, n)
    got = check(M, volume, SPACING, ms)
    for k, m in enumerate(ms):
        assert np.array_equal(records(M, volume, SPACING, [m])[0], got[k]), k
    if n == 65:
        assert (got[:, 0] == 0).any() and (got[:, 0] > 0).sum() > 20
    assert np.array_equal(records(M, volume, SPACING, []), np.zeros((0, 5), np.int64))


# ---- 4. the polygon cap, guard bytes ---------------------------------------------------------------------------------------------
def test_polygon_cap(ivxlib, volume):
    from invesalius3_amd import _lib as L
    from invesalius3_amd import measures as M
    n = L.ROI_MAX_POINTS
    t = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)
    rad = 4.0 + 1.5 * np.cos(7 * t)
    pts = [(6.0 + r * np.cos(a), 5.0 + 0.8 * r * np.sin(a), 0.0) for r, a in zip(rad, t)]
    at_cap = M.PolygonDensityMeasure("AXIAL", 3, pts)
    got = check(M, volume, SPACING, [at_cap, M.CircleDensityMeasure("AXIAL", 3, (6.0, 5.0, 0.0), (8.0, 5.0, 0.0), (6.0, 7.0, 0.0))])
    assert got[0, 0] > 50
    # one more: the library refuses it (IVX_EINVAL) and says why
    q, block = M.describe_rois(M._Grid.of(volume), SPACING, [at_cap])
    block = np.ascontiguousarray(np.concatenate([block, block[:1]]))
    q[0].n_points = n + 1
    out = np.zeros((1, 5), np.int64)
    rc = L.lib().ivx_roi_density(q, 1, L.ptr(block), len(block), L.ptr(out))
    assert rc == L.IVX_EINVAL and "%d points" % (n + 1) in L.last_error() and str(n) in L.last_error()
    with pytest.raises(TypeError):
        records(M, volume, SPACING, [M.PolygonDensityMeasure("AXIAL", 3, pts + pts[:1])])
    q[0].n_points, q[0].first_point = 3, len(block) - 2  # points past the block
    assert L.lib().ivx_roi_density(q, 1, L.ptr(block), len(block), L.ptr(out)) == L.IVX_EINVAL


def test_guard_words_around_the_records(ivxlib, volume):
    from invesalius3_amd import _lib as L
    from invesalius3_amd import measures as M
    ms = mixed_measures(M, 7)
    q, pts = M.describe_rois(M._Grid.of(volume), SPACING, ms)
    guard = np.int64(0x5A5A5A5A5A5A5A5A)
    buf = np.full(8 + 7 * 5 + 8, guard, np.int64)
    L.check(L.lib().ivx_roi_density(q, 7, L.ptr(pts), len(pts), ctypes.c_void_p(buf.ctypes.data + 64)))
    assert (buf[:8] == guard).all() and (buf[-8:] == guard).all()
    assert np.array_equal(buf[8:-8].reshape(7, 5), np.array([want_record(M, volume, SPACING, m) for m in ms], np.int64))


# ---- 5. bound arrays -----------------------------------------------------------------------------------------------------------
def test_bound_equals_unbound_with_the_stale_check(ivxlib, volume):
    from invesalius3_amd import measures as M
    from invesalius3_amd import resident
    image = np.array(volume)
    ms = orientation_measures(M) + mixed_measures(M, 12)
    unbound = records(M, image, SPACING, ms)
    r = resident.bind(image)
    try:
        resident.set_check(True)
        assert np.array_equal(records(M, image, SPACING, ms), unbound)
        image[8, 10, 12] = 5  # written and touched: the mirror follows
        r.touch(image)
        again = records(M, image, SPACING, ms)
        assert np.array_equal(again, np.array([want_record(M, image, SPACING, m) for m in ms], np.int64)) and not np.array_equal(again, unbound)
    finally:
        resident.set_check(False)
        r.release()


def test_a_bound_image_moves_no_image_byte(ivxlib, volume):
    """the copy helpers' counters: host -> device only the polygons' points (16 bytes each; the descriptors ride with the
    launch, outside the helpers), device -> host exactly 40 bytes per region, nothing served by a staging copy"""
    from invesalius3_amd import measures as M
    from invesalius3_amd import resident
    image = np.array(volume)
    r = resident.bind(image)
    try:
        for ms in (orientation_measures(M), mixed_measures(M, 65), [m for m in orientation_measures(M) if isinstance(m, M.CircleDensityMeasure)]):
            q, pts = M.describe_rois(M._Grid.of(image), SPACING, ms)
            before = resident.transfer_stats()
            got = M.roi_records(q, len(ms), pts)
            after = resident.transfer_stats()
            assert after["h2d_bytes"] - before["h2d_bytes"] == 16 * len(pts)
            assert after["d2h_bytes"] - before["d2h_bytes"] == 40 * len(ms)
            assert after["check_h2d_bytes"] == before["check_h2d_bytes"] and after["served_bytes"] == before["served_bytes"]
            assert np.array_equal(got, np.array([want_record(M, image, SPACING, m) for m in ms], np.int64))
    finally:
        r.release()


# ---- 6. the resident volume and the public calls ----------------------------------------------------------------------------
def test_device_volume_equals_the_host_call(ivxlib, volume):
    from invesalius3_amd import measures as M
    from invesalius3_amd.device import DeviceVolume
    ms = orientation_measures(M) + mixed_measures(M, 10)
    host = M.density_of(volume, SPACING, ms)
    vol = DeviceVolume(volume, spacing=SPACING)
    try:
        assert np.array_equal(vol.roi_records(ms), records(M, volume, SPACING, ms))
        assert vol.roi_density(ms) == host
        dicts = []
        for m in ms[:6]:
            dm = M.DensityMeasurement()
            dm.location, dm.type = M.LOCATIONS[m.orientation], (M.DENSITY_ELLIPSE if isinstance(m, M.CircleDensityMeasure) else M.DENSITY_POLYGON)
            dm.slice_number = m.slice_number
            m.set_measurement(dm)
        assert M.density_of(volume, SPACING, ms[:6]) == host[:6]
        dicts = [m._measurement.get_as_dict() for m in ms[:6]]
        assert vol.roi_density(dicts) == host[:6] == M.density_of(volume, SPACING, dicts)
    finally:
        vol.close()
    for m, res in zip(ms, host):
        st = R.stats(want_record(M, volume, SPACING, m))
        assert (res["min"], res["max"], res["mean"], res["std"]) == st and res["value"] == res["mean"]
        assert res["area"] == float(m.calc_area()) and res["perimeter"] == float(m.calc_perimeter())
    # recompute_measurements: stale density entries are rewritten, a linear one is left alone
    line = {"index": 9, "name": "line", "colour": [1, 0, 0], "value": 3.5, "location": 5, "type": M.LINEAR, "slice_number": 0,
            "points": [[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]], "visible": True}
    loaded = {str(k): dict(d, mean=-1.0, value=-1.0, std=-1.0) for k, d in enumerate(dicts)}
    loaded["9"] = dict(line)
    assert M.recompute_measurements(loaded, volume, SPACING) == 6 and loaded["9"] == line
    for k, d in enumerate(dicts):
        assert loaded[str(k)]["mean"] == d["mean"] == loaded[str(k)]["value"] and loaded[str(k)]["std"] == d["std"]


def test_ellipses_equal_the_reference(ivxlib):
    """min, max, mean, area, perimeter and value under ==; std under == against the exact-rational rule and within the
    pairwise-summation bound (log2(cnt) + 8) 2^-52 of the reference's float; the IndexError of np.ogrid's length quirk"""
    from invesalius3_amd import measures as M
    G = np.load(os.path.join(HERE, "golden", "ref_density.npz"))
    groups = {}
    for row, out, err in zip(G["ellipse_cases"], G["ellipse_out"], G["ellipse_raised"]):
        m = M.CircleDensityMeasure(R.ORIENTATIONS[int(row[1])], int(row[2]), tuple(row[6:9]), tuple(row[9:12]), tuple(row[12:15]))
        m.set_measurement(M.DensityMeasurement())
        if str(err):
            with pytest.raises(IndexError):
                m.calc_density(G["volume_%d" % int(row[0])], tuple(row[3:6]))
            continue
        groups.setdefault((int(row[0]), tuple(row[3:6])), []).append((m, out))
    assert len(groups) == 3
    for (v, sp), items in groups.items():
        vol = G["volume_%d" % v]
        res = M.density_of(vol, sp, [m for m, _ in items])
        for (m, out), r in zip(items, res):
            rec = want_record(M, vol, sp, m)
            assert (r["min"], r["max"], r["mean"], r["area"], r["perimeter"], r["value"]) == (out[0], out[1], out[2], out[4], out[5], out[6])
            assert r["std"] == R.stats(rec)[3]
            assert abs(r["std"] - out[3]) <= R.pairwise_bound(rec[0]) * out[3]
            dm = m._measurement
            assert (dm.min, dm.max, dm.mean, dm.std, dm.area, dm.perimeter, dm.value) == (r["min"], r["max"], r["mean"], r["std"], r["area"], r["perimeter"], r["value"])
            assert dm.points == [m.center, m.point1, m.point2]
