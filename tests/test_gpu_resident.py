"""GPU: resident host arrays.  A bound array and every view of it are served from the mirror in HBM -- the
same bytes as without the binding, and the library's own transfer counters, not a clock, say that nothing crossed the
link.  The stale check (resident.set_check) is on wherever a test wants the proof that mirror and host agree."""
import ctypes
import gc
import threading
import warnings

import numpy as np
import pytest

from conftest import synth_volume

pytestmark = pytest.mark.gpu
BONE = (226, 3071)


@pytest.fixture(autouse=True)
def _registry_returns_to_what_it_was(ivxlib):
    from invesalius3_amd import resident
    before = resident.count()
    yield
    resident.set_check(False)
    gc.collect()
    assert resident.count() == before


def _h2d():
    from invesalius3_amd import resident
    return resident.transfer_stats()["h2d_bytes"]


def _views(p):
    return {"whole": p, "interior": p[1:, 1:, 1:], "slab": p[2:4], "coronal": p[:, 3:4, :], "sagittal": p[:, :, 5:6],
            "reversed": p[::-1], "stepped": p[:, ::2], "transposed": p.transpose(2, 0, 1), "two_d": p[3, 1:, 1:],
            "stepped_x": p[:, :, ::2], "reversed_x": p[:, :, ::-1], "empty": p[3:3], "broadcast": np.broadcast_to(p[:1], p.shape)}


def _parent(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        return rng.standard_normal(shape).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)


# ---- 1. view round trips ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.uint32, np.float64])
@pytest.mark.parametrize("shape", [(6, 9, 21), (7, 10, 22), (5, 6, 32)])
def test_view_round_trips_registered_and_not(ivxlib, shape, dtype):
    """ivx_upload_strided + ivx_memcpy_d2h == np.ascontiguousarray(view); ivx_download_strided changes exactly the view's
    bytes of the parent; both with the parent bound and not, byte for byte, and bound uploads move nothing host -> device.
    ((6, 9, 21) and (7, 10, 22): `[1:, 1:, 1:]` starts misaligned and its rows are no multiple of 16 bytes; (5, 6, 32): the
    rows of `[:, :, ::2]` and `[:, :, ::-1]` are whole 16-byte chunks for every item size, the wide form of gather and scatter.)"""
    from invesalius3_amd import resident
    from invesalius3_amd.device import DeviceBuffer
    parent = _parent(shape, dtype, 1)
    buf = DeviceBuffer(parent.nbytes)
    up = {}
    for bound in (False, True):
        r = resident.bind(parent) if bound else None
        resident.set_check(bound)
        for name, v in _views(parent).items():
            h0 = _h2d()
            buf.upload_view(v)
            moved = _h2d() - h0
            got = buf.download(v.shape, v.dtype)
            assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), (name, bound)
            if bound and name != "broadcast":
                assert moved == 0, (name, moved)           # served from the mirror
            else:                                          # (a zero stride counts as not registered)
                assert moved >= v.nbytes and (moved > 0) == (v.size > 0), (name, moved)  # (a sub-box travels as its span)
            up.setdefault(name, got.tobytes())
            assert up[name] == got.tobytes()
        if r is not None:
            st = r.stats()
            assert st["hits"] == len(_views(parent)) - 2 and st["refreshes"] == 0  # all but the empty and the broadcast view
            r.release()
    # the other way: a pattern lands in the view and nowhere else
    results = {}
    for bound in (False, True):
        work = parent.copy()
        r = resident.bind(work) if bound else None
        resident.set_check(bound)
        for name, v in _views(work).items():
            if name == "broadcast":
                continue
            pattern = _parent(v.shape, dtype, 2 + len(name))
            buf.upload(pattern)
            want = work.copy()
            _views(want)[name][...] = pattern
            buf.download_view(v)
            assert np.array_equal(work.view(np.uint8), want.view(np.uint8)), (name, bound)
            results.setdefault(name, work.tobytes())
            assert results[name] == work.tobytes()
            if bound:  # the mirror got the same bytes: with the check on, a use of the whole parent compares all of them
                h0 = _h2d()
                buf.upload_view(work)
                assert _h2d() == h0
                assert np.array_equal(buf.download(work.shape, work.dtype).view(np.uint8), work.view(np.uint8)), name
        if r is not None:
            st = r.stats()
            assert st["write_throughs"] == len(_views(work)) - 2 and st["invalidations"] == 0 and st["refreshes"] == 0
            r.release()
    buf.close()


def test_a_write_that_leaves_the_range_marks_the_overlap_stale(ivxlib):
    """a dense download that covers a bound array and its neighbour cannot be written through: the overlap is uploaded
    again at the next use, exactly those bytes"""
    from invesalius3_amd import resident
    from invesalius3_amd.device import DeviceBuffer
    backing = np.zeros(4096, np.uint8)
    inner = backing[1024:3072]
    # bind() takes the allocation behind a view, so the neighbours here are two arrays of one bigger allocation: register the
    # middle of it through the C call
    h = ctypes.c_uint64(0)
    L = ivxlib
    L.check(L.lib().ivx_host_register(ctypes.c_void_p(inner.ctypes.data), inner.nbytes, ctypes.byref(h)))
    try:
        pattern = np.arange(2048, dtype=np.uint16).view(np.uint8)[:2048].copy()
        buf = DeviceBuffer(2048)
        buf.upload(pattern)
        L.check(L.lib().ivx_memcpy_d2h(ctypes.c_void_p(backing.ctypes.data + 512), buf.ptr, 2048))  # [512, 2560): half inside
        assert np.array_equal(backing[512:2560], pattern)
        st = (ctypes.c_uint64 * 8)()
        L.check(L.lib().ivx_host_stats(h.value, st))
        assert st[6] == 1 and st[4] == 0  # one invalidation, no write-through
        resident.set_check(True)
        h0 = _h2d()
        buf2 = DeviceBuffer(2048)
        buf2.upload_view(inner)
        assert _h2d() - h0 == 2560 - 1024  # the refresh of the overlap, and only that
        assert np.array_equal(buf2.download((2048,), np.uint8), inner)
        buf.close()
        buf2.close()
    finally:
        L.check(L.lib().ivx_host_release(h.value))


# ---- 2. write-through ------------------------------------------------------------------------------------------------------
def _edited_mask(shape, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros(tuple(s + 1 for s in shape), np.uint8)
    r = rng.integers(0, 40, shape)
    for k, v in ((1, 1), (2, 2), (3, 253), (4, 254), (5, 255), (6, 7)):
        m[1:, 1:, 1:][r == k] = v
    m[0, :, :] = rng.integers(0, 255, m.shape[1:])  # pad cells with something to lose
    m[:, 0, 1:] = rng.integers(0, 255, (m.shape[0], m.shape[2] - 1))
    m[1:, 0, 0] = 0
    m[2::3, 0, 0] = 2                               # some slices flagged as edited
    return m


def test_threshold_writes_through_and_the_second_call_uploads_only_flags(ivxlib):
    from invesalius3_amd import mask, resident, slice_
    shape = (12, 20, 36)
    image = synth_volume(shape, seed=3)
    m_ref = _edited_mask(shape, 4)
    m = m_ref.copy()
    # the unregistered run, on copies
    slice_.do_threshold_to_all_slices(m_ref, image.copy(), BONE)
    m_ref[1::3, 0, 0] = 0  # a new range: the reference clears the flags of the slices it wants redone
    slice_.do_threshold_to_all_slices(m_ref, image.copy(), (-200, 500))
    with slice_.bind_image(image) as ri, mask.bind_matrix(m) as rm:
        slice_.do_threshold_to_all_slices(m, image, BONE)
        for z in range(1, shape[0] + 1, 3):
            m[z, 0, 0] = 0
            rm.touch(m[z, :1, :1])
        h0 = _h2d()
        slice_.do_threshold_to_all_slices(m, image, (-200, 500))
        moved = _h2d() - h0
        assert np.array_equal(m, m_ref)  # flag and pad cells included
        # no image, no mask: the touched flag cells on the way in, the flag cells the call wrote on the way to the mirror
        assert moved == len(range(1, shape[0] + 1, 3)) + shape[0], moved
        assert ri.stats()["hits"] == 2 and ri.stats()["hit_bytes"] == 2 * image.nbytes
        assert rm.stats()["refresh_bytes"] == len(range(1, shape[0] + 1, 3))
        # the mirror equals the host after the library's own writes: with the check on every use compares them
        resident.set_check(True)
        m_ref[1:, 0, 0] = 0
        m[1:, 0, 0] = 0
        for z in range(1, shape[0] + 1):
            rm.touch(m[z, :1, :1])
        slice_.do_threshold_to_all_slices(m_ref, image.copy(), (100, 900))
        before, h0 = rm.stats(), _h2d()
        slice_.do_threshold_to_all_slices(m, image, (100, 900))
        moved, after = _h2d() - h0, rm.stats()
        assert np.array_equal(m, m_ref)
        # more than four touched cells go up packed behind their offset table (24 bytes per cell), in one copy
        assert after["refreshes"] - before["refreshes"] == shape[0] and after["refresh_bytes"] - before["refresh_bytes"] == shape[0]
        assert moved == shape[0] * (24 + 1) + shape[0], moved


# ---- 3. stale and touch ----------------------------------------------------------------------------------------------------
def test_a_forgotten_touch_is_estale_and_a_touch_uploads_exactly_the_slice(ivxlib):
    from invesalius3_amd import resident, slice_
    from invesalius3_amd._lib import StaleError
    shape = (12, 20, 36)
    image = synth_volume(shape, seed=5)
    r = slice_.bind_image(image)
    resident.set_check(True)
    assert np.array_equal(slice_.project(image, 0, slice_.PROJECTION_MaxIP), image.max(0))
    image[5] ^= 1  # (the low byte of every voxel of the slice)
    with pytest.raises(StaleError, match="IVX_ESTALE.*offset %d" % (5 * 20 * 36 * 2)):
        slice_.project(image, 0, slice_.PROJECTION_MaxIP)
    m = np.zeros(tuple(s + 1 for s in shape), np.uint8)
    with pytest.raises(RuntimeError, match="IVX_ESTALE"):
        slice_.do_threshold_to_all_slices(m, image, BONE)
    assert not m.any()
    before = r.stats()
    r.touch(image[5:6])
    slice_.do_threshold_to_all_slices(m, image, BONE)
    fresh = np.zeros_like(m)
    slice_.do_threshold_to_all_slices(fresh, image.copy(), BONE)
    assert np.array_equal(m, fresh)
    assert np.array_equal(slice_.project(image, 0, slice_.PROJECTION_MaxIP), image.max(0))
    after = r.stats()
    assert after["refresh_bytes"] - before["refresh_bytes"] == image[5:6].nbytes and after["refreshes"] - before["refreshes"] == 1
    # a touch by index means the same; one outside the array is refused
    r.touch(np.s_[7:9])
    slice_.project(image, 0, slice_.PROJECTION_MaxIP)
    assert r.stats()["refresh_bytes"] - after["refresh_bytes"] == image[7:9].nbytes
    with pytest.raises(TypeError):
        r.touch(np.zeros(4, np.int16))
    r.release()


# ---- 4. release and aliasing -----------------------------------------------------------------------------------------------
def test_release_rebind_dead_handle_and_finalizer(ivxlib):
    from invesalius3_amd import resident, slice_
    shape = (12, 20, 36)
    backing = np.empty(12 * 20 * 36 + 64, np.int16)
    backing[:] = 7
    image = backing[32:32 + 12 * 20 * 36].reshape(shape)
    image[...] = synth_volume(shape, seed=6)
    n0 = resident.count()
    r = resident.bind(image)                       # the allocation behind the view
    assert r.array is backing and r.nbytes == backing.nbytes and resident.count() == n0 + 1
    assert resident.bind(image[3:5]) is r          # the same allocation: the same registration
    assert np.array_equal(slice_.project(image, 0, slice_.PROJECTION_MaxIP), image.max(0))
    r.release()
    assert resident.count() == n0
    backing[:] = np.arange(backing.size, dtype=np.int16)   # the memory is somebody else's now
    h0 = _h2d()
    assert np.array_equal(slice_.project(image, 0, slice_.PROJECTION_MaxIP), image.max(0))
    assert _h2d() - h0 == image.nbytes
    with pytest.raises(TypeError, match="released"):       # IVX_EINVAL: no lookup by address
        r.touch()
    with pytest.raises(TypeError, match="released"):
        r.stats()
    r.release()                                             # (a second release of the object is nothing)
    r2 = resident.bind(image)
    assert r2 is not r and r2.stats()["generation"] > r.handle and resident.count() == n0 + 1
    h0 = _h2d()
    assert np.array_equal(slice_.project(image, 0, slice_.PROJECTION_MaxIP), image.max(0))
    assert _h2d() == h0
    with pytest.raises(TypeError, match="overlaps"):        # the C call refuses what bind() would have recognised
        h = ctypes.c_uint64(0)
        ivxlib.check(ivxlib.lib().ivx_host_register(ctypes.c_void_p(image.ctypes.data), 64, ctypes.byref(h)))
    del r2
    gc.collect()
    assert resident.count() == n0                           # the last reference went: released
    h0 = _h2d()
    slice_.project(image, 0, slice_.PROJECTION_MaxIP)
    assert _h2d() - h0 == image.nbytes


# ---- 5. every family sees it -----------------------------------------------------------------------------------------------
SHAPE5 = (20, 24, 40)


@pytest.fixture(scope="module")
def case5():
    image = synth_volume(SHAPE5, seed=7)
    matrix = np.zeros(tuple(s + 1 for s in SHAPE5), np.uint8)
    matrix[1:, 1:, 1:] = np.where((image >= BONE[0]) & (image <= BONE[1]), 255, 0)
    matrix[1:, 1:, 1:][11, 15, 18:20] = 0      # a hole for fill_holes_auto, two voxels deep inside the bone
    matrix[1:, 0, 0] = 1
    z, y, x = np.unravel_index(int(np.argmax(image)), image.shape)
    assert (z, y, x) == (12, 17, 26) and matrix[1:, 1:, 1:][z, y, x] == 255
    image.setflags(write=False)
    matrix.setflags(write=False)
    return image, matrix, (int(x), int(y), int(z))


def _bound_equals_unbound(fn, image0, matrix0, other_bytes=0):
    """fn(image, matrix) -> arrays; run on private copies unbound, then bound with the check on; the results and what the
    call did to its arrays are the same bytes, and bound it uploads nothing but `other_bytes` (arrays that are nobody's
    image or matrix: markers, a selection) and small arguments"""
    from invesalius3_amd import mask, resident, slice_
    img_a, mat_a = image0.copy(), matrix0.copy()
    h0 = _h2d()
    want = fn(img_a, mat_a)
    unbound = _h2d() - h0
    img_b, mat_b = image0.copy(), matrix0.copy()
    with slice_.bind_image(img_b) as ri, mask.bind_matrix(mat_b) as rm:
        resident.set_check(True)
        h0 = _h2d()
        got = fn(img_b, mat_b)
        bound = _h2d() - h0
        hits = ri.stats()["hits"] + rm.stats()["hits"]
        resident.set_check(False)
    assert len(want) == len(got)
    for a, b in zip(want, got):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert img_a.tobytes() == img_b.tobytes() and mat_a.tobytes() == mat_b.tobytes()
    assert hits >= 1
    assert other_bytes <= bound <= other_bytes + 1024, (bound, unbound)
    assert unbound > bound, (bound, unbound)
    return want


def test_family_floodfill_threshold(ivxlib, case5):
    from invesalius3_amd import invesalius_rs as rs
    from invesalius3_amd.mask import _structure
    image, matrix, seed = case5

    def out_of_place(img, mat):
        mat[1:, 1:, 1:] = 0  # (numpy wrote the bound matrix ...)
        from invesalius3_amd import resident
        resident.touch(mat[1:, 1:, 1:])  # ... and says so
        rs.floodfill_threshold(img, [seed], BONE[0], BONE[1], 254, _structure(3, 3), mat[1:, 1:, 1:])
        return (mat[1:, 1:, 1:].copy(),)

    # the touched interior goes up once more (the refresh) on its way into the call
    (out,) = _bound_equals_unbound(out_of_place, image, matrix, other_bytes=matrix.nbytes - matrix[0].nbytes - matrix[0, 0].nbytes - 1)
    assert out[seed[2], seed[1], seed[0]] == 254 and 0 < np.count_nonzero(out) < out.size

    def in_place(img, mat):
        rs.floodfill_threshold_inplace(mat[1:, 1:, 1:], [seed], 253, 255, 7, _structure(3, 1))
        return (mat[1:, 1:, 1:].copy(),)

    (out,) = _bound_equals_unbound(in_place, image, matrix)
    assert out[seed[2], seed[1], seed[0]] == 7


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_family_projections_of_slabs(ivxlib, case5, axis, k):
    from invesalius3_amd import invesalius_rs as rs
    from invesalius3_amd import slice_
    image, matrix, _ = case5

    def projections(img, mat):
        sl = [slice(None)] * 3
        sl[axis] = slice(7, 7 + k)
        slab = img[tuple(sl)]
        oshape = tuple(s for i, s in enumerate(slab.shape) if i != axis)
        mida, fcm = np.zeros(oshape, np.int16), np.zeros(oshape, np.int16)
        rs.mida(slab, axis, 300, 300, mida)
        rs.fast_countour_mip(slab, 1.0, axis, 300, 300, 0, fcm)
        return [slice_.project(slab, axis, p) for p in (slice_.PROJECTION_MaxIP, slice_.PROJECTION_MinIP, slice_.PROJECTION_MeanIP)] + [mida, fcm]

    want = _bound_equals_unbound(projections, image, matrix)
    sl = [slice(None)] * 3
    sl[axis] = slice(7, 7 + k)
    assert np.array_equal(want[0], image[tuple(sl)].max(axis))


def test_family_marching_cubes(ivxlib, case5):
    from invesalius3_amd import surface_process as sp
    image, matrix, _ = case5

    def surfaces(img, mat):
        return (sp.marching_cubes(img, (0.5, 0.5, 2.0), BONE, pad_value=float(np.iinfo(np.int16).min)),
                sp.marching_cubes(mat[1:, 1:, 1:], (0.5, 0.5, 2.0), [127]))

    a, b = _bound_equals_unbound(surfaces, image, matrix)
    assert len(a) > 0 and len(b) > 0


@pytest.mark.parametrize("algorithm", ["Watershed", "Watershed IFT"])
def test_family_do_watershed(ivxlib, case5, tmp_path, algorithm):
    from invesalius3_amd import watershed_process as wp
    from invesalius3_amd.mask import _structure
    image, matrix, (x, y, z) = case5
    markers = np.zeros(SHAPE5, np.int16)
    markers[z, y, x] = 1
    markers[0, 0, 0] = markers[-1, -1, -1] = 2
    count = [0]

    def flood(img, mat):
        count[0] += 1
        tfile = str(tmp_path / ("labels_%d.dat" % count[0]))
        np.zeros(SHAPE5, np.uint8).tofile(tfile)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            wp.do_watershed(img, markers, tfile, SHAPE5, _structure(3, 1), algorithm, (3, 3, 3), True, 300, 400, None)
        return (np.fromfile(tfile, np.uint8).reshape(SHAPE5),)

    (labels,) = _bound_equals_unbound(flood, image, matrix, other_bytes=markers.nbytes)
    assert set(np.unique(labels)) <= {0, 1, 2} and (labels == 1).any() and (labels == 2).any()


def test_family_filter_devicevolume_and_fill_holes(ivxlib, case5):
    from invesalius3_amd import mask, slice_
    from invesalius3_amd.device import DeviceVolume
    image, matrix, _ = case5
    (f,) = _bound_equals_unbound(lambda img, mat: (slice_.apply_image_filter(img, 0, 1.0),), image, matrix)
    assert f.dtype == np.int16 and f.shape == image.shape and not np.array_equal(f, image)

    def volume(img, mat):
        with DeviceVolume(img) as vol:
            vol.mask.upload_view(mat[1:, 1:, 1:])
            vol.sync()
            return vol.image.download(vol.shape, np.int16), vol.download_mask()

    a, b = _bound_equals_unbound(volume, image, matrix)
    assert np.array_equal(a, image) and np.array_equal(b, matrix[1:, 1:, 1:])

    def holes(img, mat):
        changed = mask.fill_holes_auto(mat, "3D", 6, "AXIAL", 0, 1000)
        changed2 = mask.fill_holes_auto(mat, "2D", 4, "SAGITAL", 9, 1000)
        return (np.array([changed, changed2]), mat.copy())

    flags, filled = _bound_equals_unbound(holes, image, matrix)
    assert flags[0] and (filled[1:, 1:, 1:][11, 15, 18:20] == 254).all()


@pytest.mark.parametrize("method", ["threshold", "dynamic", "confidence"])
def test_family_do_3d_seg(ivxlib, case5, method):
    from invesalius3_amd import styles
    image, matrix, seed = case5

    def click(img, mat):
        ok = styles.do_3d_seg(img, mat, seed, method=method, con_3d=6, fill_value=254, t0=BONE[0], t1=BONE[1], dev_min=400,
                              dev_max=400, threshold_range=BONE)
        return (np.array([ok]), mat.copy())

    # the confidence mode uploads its selection volume (one byte per voxel), built on the host per call
    ok, out = _bound_equals_unbound(click, image, matrix, other_bytes=image.size if method == "confidence" else 0)
    assert ok[0] and (out[1:, 1:, 1:] == 254).any()


def test_family_two_d_outputs_into_a_bound_array(ivxlib, case5):
    """the 2-D form: a projection written into a view of a bound 2-D array (download_strided2 -> the general scatter behind
    an axis of length 1) reaches the mirror too -- a checked use of the whole array afterwards compares every byte"""
    from invesalius3_amd import invesalius_rs as rs
    from invesalius3_amd import resident
    from invesalius3_amd.device import DeviceBuffer
    image, _, _ = case5
    want = np.zeros(SHAPE5[1:], np.int16)
    rs.mida(image, 0, 300, 300, want)
    canvas = np.full((30, 50), -7, np.int16)
    canvas_t = np.full((44, 28), -7, np.int16)
    buf = DeviceBuffer(canvas.nbytes)
    with resident.bind(canvas) as rc, resident.bind(canvas_t) as rt:
        resident.set_check(True)
        rs.mida(image, 0, 300, 300, canvas[2:26, 3:43])          # a sub-box: rows with a pitch
        rs.mida(image, 0, 300, 300, canvas_t[1:41, 2:26].T)      # transposed: no contiguous rows
        assert rc.stats()["write_throughs"] == 1 and rt.stats()["write_throughs"] == 1
        assert rc.stats()["invalidations"] == 0 and rt.stats()["invalidations"] == 0
        for arr in (canvas, canvas_t):
            h0 = _h2d()
            buf.upload_view(arr)                                  # checked: host == mirror, byte for byte
            assert _h2d() == h0
            assert np.array_equal(buf.download(arr.shape, arr.dtype), arr)
    buf.close()
    assert np.array_equal(canvas[2:26, 3:43], want) and np.array_equal(canvas_t[1:41, 2:26].T, want)
    edge = np.ones(canvas.shape, bool)
    edge[2:26, 3:43] = False
    assert (canvas[edge] == -7).all()


# ---- 6. past the staging threshold -----------------------------------------------------------------------------------------
def test_past_the_staging_threshold(ivxlib, monkeypatch):
    """4.7 MB of int16: dense downloads of 4 MB and more can take the page-locked lanes (forced here, since the pages of
    these arrays have been written); the mirror still gets what the host got"""
    from invesalius3_amd import invesalius_rs as rs
    from invesalius3_amd import mask, resident, slice_
    from invesalius3_amd.mask import _structure
    shape = (64, 128, 288)
    image = synth_volume(shape, seed=8)
    assert image.nbytes >= 4 << 20
    z, y, x = (int(v) for v in np.unravel_index(int(np.argmax(image)), shape))
    monkeypatch.setenv("IVX_D2H_LANES", "1")

    def run(img, mat):
        slice_.do_threshold_to_all_slices(mat, img, BONE)
        rs.floodfill_threshold_inplace(mat[1:, 1:, 1:], [(x, y, z)], 255, 255, 254, _structure(3, 1))
        rs.floodfill_threshold_inplace(img, [(x, y, z)], BONE[0], BONE[1], -1000, _structure(3, 1))  # a dense 4.7 MB each way

    img_a, mat_a = image.copy(), np.zeros(tuple(s + 1 for s in shape), np.uint8)
    run(img_a, mat_a)
    assert (mat_a == 254).any() and (img_a != image).any()
    img_b, mat_b = image.copy(), np.zeros(tuple(s + 1 for s in shape), np.uint8)
    with slice_.bind_image(img_b) as ri, mask.bind_matrix(mat_b) as rm:
        h0 = _h2d()
        run(img_b, mat_b)
        assert _h2d() - h0 == shape[0]  # the flag cells the threshold wrote
        assert np.array_equal(img_a, img_b) and np.array_equal(mat_a, mat_b)
        assert ri.stats()["write_through_bytes"] == image.nbytes and ri.stats()["invalidations"] == 0
        assert rm.stats()["invalidations"] == 0 and rm.stats()["refreshes"] == 0
        resident.set_check(True)  # mirror == host, for both, after all of it
        assert np.array_equal(slice_.project(img_b, 0, slice_.PROJECTION_MaxIP), img_b.max(0))
        assert np.array_equal(slice_.project(mat_b, 0, slice_.PROJECTION_MaxIP), mat_b.max(0))


# ---- 7. two host threads ---------------------------------------------------------------------------------------------------
def test_two_host_threads_on_one_bound_image(ivxlib):
    from invesalius3_amd import invesalius_rs as rs
    from invesalius3_amd import resident, slice_
    from invesalius3_amd.mask import _structure
    shape = (20, 24, 40)
    image = synth_volume(shape, seed=9)
    z, y, x = (int(v) for v in np.unravel_index(int(np.argmax(image)), shape))
    want_out = np.zeros(shape, np.uint8)
    rs.floodfill_threshold(image.copy(), [(x, y, z)], BONE[0], BONE[1], 1, _structure(3, 3), want_out)
    results, errors = {}, []

    def mips():
        try:
            results["mip"] = [slice_.project(image[:, a:a + 5], 1, slice_.PROJECTION_MaxIP) for a in range(0, 16)]
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    def floods():
        try:
            outs = []
            for _ in range(4):
                out = np.zeros(shape, np.uint8)
                rs.floodfill_threshold(image, [(x, y, z)], BONE[0], BONE[1], 1, _structure(3, 3), out)
                outs.append(out)
            results["flood"] = outs
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    with slice_.bind_image(image) as r:
        resident.set_check(True)
        h0 = _h2d()
        threads = [threading.Thread(target=mips), threading.Thread(target=floods)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert _h2d() - h0 <= 4 * want_out.nbytes + 1024  # the floods' zeroed `out` arrays (they are read: barriers), no image
        assert r.stats()["hits"] == 16 + 4
    for a, got in enumerate(results["mip"]):
        assert np.array_equal(got, image[:, a:a + 5].max(1))
    for out in results["flood"]:
        assert np.array_equal(out, want_out)


# ---- 8. device key ---------------------------------------------------------------------------------------------------------
def test_another_device_treats_the_array_as_not_registered(ivxlib):
    from invesalius3_amd import slice_
    if ivxlib.device_count() < 2:
        pytest.skip("one device visible")
    image = synth_volume((12, 20, 36), seed=10)
    with slice_.bind_image(image) as r:
        try:
            ivxlib.set_device(1)
            h0 = _h2d()
            assert np.array_equal(slice_.project(image, 0, slice_.PROJECTION_MaxIP), image.max(0))
            assert _h2d() - h0 == image.nbytes and r.stats()["hits"] == 0
        finally:
            ivxlib.set_device(0)
        h0 = _h2d()
        assert np.array_equal(slice_.project(image, 0, slice_.PROJECTION_MaxIP), image.max(0))
        assert _h2d() == h0 and r.stats()["hits"] == 1
