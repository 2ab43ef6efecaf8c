"""GPU: the image geometry tools -- flip, swap axes and the gantry-tilt correction -- against numpy, live scipy and
the reference's own output (tests/golden/ref_imagetools.npz), all under np.array_equal; what they leave of masks and of a
DeviceVolume's derived state; and that a bound image crosses the link once, device to host, and a bound mask not at all."""
import ctypes
import gc
import itertools

import numpy as np
import pytest
from scipy.ndimage import shift

import _imagegeo_cases as C

pytestmark = pytest.mark.gpu
REV = (np.s_[::-1], np.s_[:, ::-1], np.s_[:, :, ::-1])
LENGTHS = (1, 2, 3, 8, 9)                       # of the flipped axis: nothing to do, one pair, a middle line, even, odd
WIDTHS = (1, 2, 7, 8, 9, 63, 64, 65, 129)       # below one 16-byte chunk, odd, whole chunks (an even and an odd count), tails
PHANTOMS = {"disc": C.disc_phantom, "slice0": C.slice0_min_phantom, "wave": lambda: C.disc_phantom((5, 64, 64), seed=13)}
THR = (200, 3071)


@pytest.fixture(autouse=True)
def _registry_returns_to_what_it_was(ivxlib):
    from invesalius3_amd import resident
    before = resident.count()
    yield
    resident.set_check(False)
    gc.collect()
    assert resident.count() == before


def _rand(shape, dtype, seed=0):
    rng = np.random.default_rng(seed + sum(shape))
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 256, size=shape).astype(np.uint8)
    return rng.integers(-32768, 32768, size=shape).astype(dtype)


def _xfer():
    from invesalius3_amd import resident
    s = resident.transfer_stats()
    return s["h2d_bytes"], s["d2h_bytes"]


def _mirror_bytes(a):
    """what the device holds for a bound array: an upload of it is served from the mirror"""
    from invesalius3_amd.device import DeviceBuffer
    buf = DeviceBuffer(a.nbytes)
    try:
        buf.upload_view(a)
        return buf.download(a.shape, a.dtype)
    finally:
        buf.close()


def _padded_mask(shape, seed=1):
    """a padded matrix with content and all three kinds of flag"""
    m = np.random.default_rng(seed).choice(np.array([0, 1, 2, 253, 254, 255], np.uint8), size=tuple(s + 1 for s in shape))
    m[1:, 0, 0], m[0, 1:, 0], m[0, 0, 1:] = 1, 2, 1
    return m


# ---- flip ----------------------------------------------------------------------------------------------------------------------------
def _flip_shapes(axis):
    if axis == 2:
        return [(3, 2, w) for w in WIDTHS] + [(1, 1, 16), (2, 3, 24), (1, 5, 130)]
    out = []
    for n, w in itertools.product(LENGTHS, WIDTHS):
        out.append((n, 3, w) if axis == 0 else (2, n, w))
    return out


@pytest.mark.parametrize("dtype", [np.int16, np.uint8])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_flip_equals_numpy_and_twice_is_the_identity(ivxlib, axis, dtype):
    from invesalius3_amd import slice_
    for shape in _flip_shapes(axis):
        a = _rand(shape, dtype)
        m = a.copy()
        slice_.flip_volume(m, axis)
        assert np.array_equal(m, a[REV[axis]]), (shape, axis)
        slice_.flip_volume(m, axis)
        assert np.array_equal(m, a), (shape, axis)


@pytest.mark.parametrize("dtype", [np.float64, np.uint16, np.int32])
def test_flip_of_the_other_item_sizes(ivxlib, dtype):
    from invesalius3_amd import slice_
    for shape, axis in itertools.product([(3, 5, 7), (2, 4, 8), (9, 2, 33)], range(3)):
        a = (np.random.default_rng(3).random(shape) * 1000).astype(dtype)
        m = a.copy()
        slice_.flip_volume(m, axis)
        assert np.array_equal(m, a[REV[axis]])


@pytest.mark.parametrize("dtype", [np.int16, np.uint8])
def test_device_flip_of_a_block_that_is_not_16_byte_aligned(ivxlib, dtype):
    """the device form on a block that starts one element into an allocation: no 16-byte chunk path may be taken"""
    from invesalius3_amd import _lib as L
    from invesalius3_amd.device import DeviceBuffer
    isz = np.dtype(dtype).itemsize
    for shape, axis in itertools.product([(4, 6, 64), (5, 3, 16), (2, 9, 40)], range(3)):
        a = _rand(shape, dtype, seed=9)
        guard = np.concatenate([np.array([77], dtype), a.reshape(-1), np.array([88], dtype)])
        buf = DeviceBuffer(guard.nbytes)
        try:
            buf.upload(guard)
            L.check(L.lib().ivx_dev_image_flip(buf.at(isz), *shape, isz, axis, None), "flip")
            L.synchronize()
            got = buf.download(guard.shape, dtype)
        finally:
            buf.close()
        assert got[0] == 77 and got[-1] == 88
        assert np.array_equal(got[1:-1].reshape(shape), a[REV[axis]]), (shape, axis)


def test_flip_versions_and_views(ivxlib):
    from invesalius3_amd import slice_
    a, v = _rand((5, 6, 9), np.int16), _rand((5, 6, 9), np.int16, seed=4)
    m, mv = a.copy(), v.copy()
    slice_.flip_volume(m, 1, versions=[("original", m), ("Filtered 1", mv)])
    assert np.array_equal(m, a[:, ::-1]) and np.array_equal(mv, v[:, ::-1])  # (the matrix itself is not flipped twice)
    g = C.golden()
    for axis in range(3):  # the reference's own output
        m, mv = g["geo_in"].copy(), g["geo_version_in"].copy()
        slice_.flip_volume(m, axis, versions=[mv])
        assert np.array_equal(m, g["flip_out_%d" % axis]) and np.array_equal(mv, g["flip_version_out_%d" % axis])
    big = _rand((6, 8, 20), np.int16, seed=5)
    view, want = big[1:5, 2:7, 3:19], big.copy()
    want[1:5, 2:7, 3:19] = want[1:5, 2:7, 3:19][:, :, ::-1]
    slice_.flip_volume(view, 2)  # a sub-box: the bytes between its rows stay
    assert np.array_equal(big, want)


# ---- swap ----------------------------------------------------------------------------------------------------------------------------
SWAP_SHAPES = [(1, 2, 31), (2, 31, 32), (31, 32, 33), (32, 33, 65), (33, 65, 1), (65, 1, 2), (65, 33, 31), (1, 1, 1), (2, 65, 65),
               (64, 64, 3), (3, 130, 64), (65, 2, 129)]


@pytest.mark.parametrize("pair", [(2, 1), (2, 0), (1, 0)])
def test_swap_equals_numpy_in_either_order(ivxlib, pair):
    from invesalius3_amd import slice_
    sp = (0.5, 0.75, 2.0)
    for shape in SWAP_SHAPES:
        for dtype in (np.int16, np.uint8) if shape[0] > 2 else (np.int16,):
            a = _rand(shape, dtype, seed=2)
            want = np.array(a.swapaxes(*pair))
            for axes in (pair, pair[::-1]):
                new, nsp, masks, versions = slice_.swap_volume_axes(a, axes, sp)
                assert new.shape == want.shape and new.flags["C_CONTIGUOUS"] and np.array_equal(new, want), (shape, axes)
                assert nsp == slice_.swapped_spacing(sp, pair) and masks == [] and versions == []
    a = (np.random.default_rng(8).random((5, 33, 70)) * 100).astype(np.float64)  # the element-size-generic path
    assert np.array_equal(slice_.swap_volume_axes(a, pair, sp)[0], np.array(a.swapaxes(*pair)))


def test_swap_equals_the_reference(ivxlib):
    from invesalius3_amd import slice_
    g = C.golden()
    for key in ("21", "20", "10"):
        axes = (int(key[0]), int(key[1]))
        mask = _padded_mask(g["geo_in"].shape)
        new, sp, masks, versions = slice_.swap_volume_axes(g["geo_in"], axes, tuple(g["geo_spacing"]), masks=[mask],
                                                           versions=[("Filtered 1", g["geo_version_in"])])
        assert np.array_equal(new, g["swap_out_" + key]) and np.array_equal(versions[0], g["swap_version_out_" + key])
        assert sp == tuple(g["swap_spacing_" + key])
        assert masks[0].shape == tuple(g["swap_mask_shape_" + key]) and masks[0].dtype == np.uint8 and not masks[0].any()


# ---- gantry tilt ---------------------------------------------------------------------------------------------------------------------
def _shift_chain(vol, shifts):
    """the tool's loop over live scipy with given shifts"""
    cvals = []
    for n, s in enumerate(shifts):
        cvals.append(int(vol.min()))
        vol[n] = shift(vol[n], (s, 0), cval=cvals[-1])
    return cvals


def _abi_tilt(vol, shifts):
    from invesalius3_amd import _lib as L
    shifts = np.ascontiguousarray(shifts, np.float64)
    cvals = np.zeros(len(shifts), np.int32)
    L.check(L.lib().ivx_image_fix_gantry_tilt(L.ptr(vol), L.i64(vol.shape), L.i64(vol.strides), L.ptr(shifts), L.ptr(cvals)), "tilt")
    return [int(v) for v in cvals]


def test_tilt_cpu_fixtures_through_the_c_abi(ivxlib):
    cases = [(C.fixture_slice(), C.SHIFTS)]
    for h in (2, 3, 4):
        cases.append((C.small_slice(h), (0.0, -0.37, 0.3, -1.0, 1.0, -1.5, 2.0, -3.0) + ((0.5,) if h > 2 else ())))
    cases.append((C.small_slice(1, w=7), (0.0, 0.25, -1.0)))
    for s, shifts in cases:
        for order in (shifts, shifts[::-1]):  # (the chain of fill values differs with the order)
            vol = np.stack([s] * len(order))
            want = vol.copy()
            want_cvals = _shift_chain(want, order)
            assert _abi_tilt(vol, order) == want_cvals
            assert np.array_equal(vol, want), (s.shape, order)
    vol = np.stack([C.fixture_slice()] * 3)
    assert _abi_tilt(vol, (0.0, 0.0, 0.0)) and np.array_equal(vol, np.stack([C.fixture_slice()] * 3))  # shift 0: the input


@pytest.mark.parametrize("name", sorted(PHANTOMS))
@pytest.mark.parametrize("tilt", C.TILTS)
def test_tilt_equals_the_reference_and_live_scipy(ivxlib, name, tilt):
    from invesalius3_amd import _lib as L
    from invesalius3_amd import slice_
    from invesalius3_amd.device import DeviceVolume
    vol = PHANTOMS[name]()
    want = vol.copy()
    want_cvals = C.scipy_fix_gantry_tilt(want, C.PHANTOM_SPACING, tilt)
    assert np.array_equal(want, C.golden()["tilt_out_%s_%g" % (name, tilt)])
    m = vol.copy()
    cvals = slice_.fix_gantry_tilt(m, C.PHANTOM_SPACING, tilt)
    assert np.array_equal(m, want) and [int(v) for v in cvals] == want_cvals
    if tilt == 0.0:
        assert np.array_equal(m, vol)
    # the resident form, in one launch and one slice at a time: the launch shape changes nothing
    nb = ctypes.c_size_t(0)
    d, h, w = vol.shape
    L.check(L.lib().ivx_image_tilt_scratch_bytes(d, 1, 1, ctypes.byref(nb)))
    one_slice = nb.value - 8 + h * w * 8
    for scratch in (None, one_slice, one_slice + 2 * h * w * 8):
        with DeviceVolume(vol, spacing=C.PHANTOM_SPACING) as dv:
            got_cvals = dv.fix_gantry_tilt(tilt, scratch_bytes=scratch)
            dv.sync()
            assert np.array_equal(dv.image.download(vol.shape, np.int16), want), scratch
            assert [int(v) for v in got_cvals] == want_cvals


# ---- masks and derived state ---------------------------------------------------------------------------------------------------------
def _tools():
    from invesalius3_amd import slice_
    sp = C.PHANTOM_SPACING

    def flip(img, masks):
        slice_.flip_volume(img, 1, masks=masks)
        return img, [m if isinstance(m, np.ndarray) else m.matrix for m in masks], img[:, ::-1]

    def swap(img, masks):
        new, _, new_masks, _ = slice_.swap_volume_axes(img, (2, 0), sp, masks=masks)
        return new, new_masks, None

    def tilt(img, masks):
        slice_.fix_gantry_tilt(img, sp, 11.5, masks=masks)
        return img, list(masks), None

    return {"flip": flip, "swap": swap, "tilt": tilt}


@pytest.mark.parametrize("tool", ["flip", "swap", "tilt"])
def test_bound_mask_is_zero_after_each_tool_and_the_next_threshold_is_fresh(ivxlib, tool):
    from invesalius3_amd import mask as mk
    from invesalius3_amd import resident, slice_
    img0 = C.disc_phantom((9, 20, 24), seed=21)
    want_img = img0.copy()
    if tool == "flip":
        want_img = np.array(want_img[:, ::-1])
    elif tool == "swap":
        want_img = np.array(want_img.swapaxes(2, 0))
    else:
        C.scipy_fix_gantry_tilt(want_img, C.PHANTOM_SPACING, 11.5)
    img, mask = img0.copy(), _padded_mask(img0.shape)
    r_img, r_mask = slice_.bind_image(img), mk.bind_matrix(mask)
    new_img = m = None
    try:
        slice_.do_threshold_to_all_slices(mask, img, THR)  # (flagged slices stay: the mask holds a mix)
        resident.set_check(True)
        new_img, new_masks, _ = _tools()[tool](img, [mask])
        m = new_masks[0]
        assert np.array_equal(new_img, want_img)
        assert m.shape == tuple(s + 1 for s in want_img.shape) and not m.any()       # host
        assert resident.find(m) is not None and not _mirror_bytes(m).any()            # device, flag planes included
        assert resident.find(new_img) is not None and np.array_equal(_mirror_bytes(new_img), want_img)
        # what follows equals a fresh run on the transformed image
        fresh = np.zeros_like(m)
        got_slice = slice_.get_mask_slice(m, new_img, "CORONAL", 3, THR)
        want_slice = slice_.get_mask_slice(fresh, want_img.copy(), "CORONAL", 3, THR)
        assert np.array_equal(got_slice, want_slice) and np.array_equal(m, fresh)
        slice_.do_threshold_to_all_slices(m, new_img, THR)
        slice_.do_threshold_to_all_slices(fresh, want_img.copy(), THR)
        assert np.array_equal(m, fresh) and (m[1:, 1:, 1:] == 255).any()
        resident.set_check(False)
    finally:
        resident.set_check(False)
        for a in (new_img, m):
            r = resident.find(a) if a is not None else None
            if r is not None:
                r.release()
        r_img.release()
        r_mask.release()


def _derived(dv):
    from invesalius3_amd import _lib as L
    from invesalius3_amd.device import DeviceBuffer
    dv.threshold(*THR)
    tris = dv.marching_cubes(from_binary=True, download=True).copy()
    out = DeviceBuffer(dv.dy * dv.dx * 2)
    try:
        dv.project(0, L.MIP_MAX, out)
        rng = dv.image_range()
        dv.sync()
        return tris, out.download((dv.dy, dv.dx), np.int16), rng.download((2,), np.float32), dv.download_mask()
    finally:
        out.close()


@pytest.mark.parametrize("tool", ["flip0", "flip1", "flip2", "swap21", "swap20", "swap10", "tilt"])
def test_device_volume_drops_every_stale_record(ivxlib, tool):
    """threshold, marching cubes, projection and range before the tool leave their records and caches behind; after it the
    same calls equal those of a fresh volume made from numpy's transformed image"""
    from invesalius3_amd.device import DeviceVolume
    sp = (0.5, 0.75, 2.0)
    img = C.disc_phantom((10, 24, 64), seed=22)  # (64 wide: the fused threshold with its plane and per-word records runs)
    img[2, 3, 5], img[7, 20, 60] = -3000, 3000   # the range's two ends, which a flip moves and a swap keeps
    with DeviceVolume(img, spacing=sp) as dv:
        before = _derived(dv)
        assert len(before[0]) > 0
        if tool.startswith("flip"):
            axis = int(tool[4])
            dv.flip(axis)
            want_img, want_sp = np.array(img[REV[axis]]), sp
        elif tool.startswith("swap"):
            a, b = int(tool[4]), int(tool[5])
            dv.swap_axes((a, b))
            want_img = np.array(img.swapaxes(a, b))
            want_sp = {"21": (sp[1], sp[0], sp[2]), "20": (sp[2], sp[1], sp[0]), "10": (sp[0], sp[2], sp[1])}[tool[4:]]
        else:
            dv.fix_gantry_tilt(11.5)
            want_img, want_sp = img.copy(), sp
            C.scipy_fix_gantry_tilt(want_img, sp, 11.5)
        assert dv.shape == want_img.shape and dv.spacing == want_sp
        assert not dv.download_mask().any() and not dv.download_out_mask().any()
        dv.sync()
        assert np.array_equal(dv.image.download(dv.shape, np.int16), want_img)
        got = _derived(dv)
        with DeviceVolume(want_img, spacing=want_sp) as fresh:
            want = _derived(fresh)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w)
        # a region growing on the new geometry (its planes and scratch are the new shape's)
        z, y, x = (int(v) for v in np.unravel_index(int(np.argmax(want_img)), want_img.shape))
        dv.zero_out_mask()
        dv.region_grow([(x, y, z)], 1000, 3071, np.ones((3, 3, 3), np.uint8), fill=1, select_value=None)
        assert dv.download_out_mask()[z, y, x] == 1


# ---- resident ------------------------------------------------------------------------------------------------------------------------
def test_bound_and_unbound_return_the_same_bytes_and_a_bound_image_goes_down_once(ivxlib):
    from invesalius3_amd import mask as mk
    from invesalius3_amd import resident, slice_
    img0 = C.disc_phantom((12, 40, 48), seed=23)
    sp = C.PHANTOM_SPACING
    for tool, run in _tools().items():
        plain = run(img0.copy(), [])[0]
        img, mask = img0.copy(), _padded_mask(img0.shape)
        r_img, r_mask = slice_.bind_image(img), mk.bind_matrix(mask)
        new_img = m = None
        try:
            up0, down0 = _xfer()
            new_img, new_masks, _ = run(img, [mask])
            m = new_masks[0]
            up1, down1 = _xfer()
            assert up1 - up0 == 0, (tool, up1 - up0)                    # no image byte and no mask byte host -> device
            assert down1 - down0 == img0.nbytes, (tool, down1 - down0)  # the image once device -> host, the mask not at all
            assert np.array_equal(new_img, plain) and not m.any()
            resident.set_check(True)  # host and mirror agree byte for byte, for the image and the mask
            assert np.array_equal(slice_.project(new_img, 0, slice_.PROJECTION_MaxIP), plain.max(axis=0))
            assert not slice_.project(m[1:, 1:, 1:], 0, slice_.PROJECTION_MaxIP).any()
            resident.set_check(False)
            up2, _ = _xfer()
            slice_.project(new_img, 0, slice_.PROJECTION_MaxIP)  # the next use finds the image in HBM
            assert _xfer()[0] == up2
            if tool != "swap":
                assert resident.find(new_img) is r_img and resident.find(m) is r_mask  # the bindings stayed valid
                assert r_img.stats()["refresh_bytes"] == 0
            else:
                assert r_img._released and r_mask._released and resident.find(img) is None
        finally:
            for a in (new_img, m):
                r = resident.find(a) if a is not None else None
                if r is not None:
                    r.release()
            r_img.release()
            r_mask.release()


def test_stale_check_still_catches_a_forgotten_touch_after_a_flip(ivxlib):
    from invesalius3_amd import _lib as L
    from invesalius3_amd import resident, slice_
    img = C.disc_phantom((6, 16, 16), seed=24)
    with slice_.bind_image(img):
        slice_.flip_volume(img, 0)
        img[1, 2, 3] += 1  # a numpy write without touch
        resident.set_check(True)
        with pytest.raises(L.StaleError):
            slice_.project(img, 0, slice_.PROJECTION_MaxIP)
        resident.set_check(False)
