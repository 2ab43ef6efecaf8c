"""Image filters (k_filter.hip) where the other filter tests do not reach, bit for bit against live scipy:
A. the LDS-fit switch of sym_pass() and the global-memory pass k_sym_pass behind it, up to the radius cap;
B. more than one k_sym_x row tile, k_sym_zy tile and k_box_pass segment, with partial last ones, rows wider than 256;
C. sigma <= 1e-15 (no pass at all), int16's two ends, 2-D runs in which some slices are flat;
D. the same through the resident DeviceVolume.filter_image.
Every comparison is np.array_equal plus a dtype check: that is the contract k_filter.hip states.  Each case asserts,
from the constants restated below, which kernel and branch it is on, so that a retune fails here instead of silently
un-testing a path."""
import ctypes
import functools

import numpy as np
import pytest

from _filters_ref import AXIS, _fn, _ref, _ref_2d

pytestmark = pytest.mark.gpu

# Restated from k_filter.hip: the row tile of k_sym_x, the z / y tile of k_sym_zy (64 x-lanes wide), the dynamic LDS
# sym_pass() allows a block (`<= 65536`), scipy's kernel radius, IVX_FILTER_MAX_RADIUS; the z / y segment of k_box_pass,
# the x stride of k_seg_minmax_rows and the row budget of seg_minmax() (`rpb = max(1, 8192 / nx)`).
XT, LT, LANES, LDS_LIMIT, MAX_RADIUS = 1024, 64, 64, 65536, 255
BOX_SEG, MINMAX_STRIDE, MINMAX_ROW_BUDGET = 64, 256, 8192
I16, F64 = 2, 8  # item sizes of the pass inputs: int16 (Gaussian, despeckle, the first float64 pass), float64 (the later ones)

MODES = [("3D", "Axial"), ("2D", "Axial"), ("2D", "Coronal"), ("2D", "Sagittal")]


def _sid(shape):
    return "x".join(str(s) for s in shape)


def radius(sigma):
    return int(4.0 * sigma + 0.5)


def zy_tile_bytes(r, itemsize):
    return (LT + 2 * r) * LANES * itemsize


def zy_in_lds(r, itemsize):
    """sym_pass() along z or y: k_sym_zy when True, the global-memory k_sym_pass when False"""
    return zy_tile_bytes(r, itemsize) <= LDS_LIMIT


def x_in_lds(r, itemsize):
    return (XT + 2 * r) * itemsize <= LDS_LIMIT


def cdiv(a, b):
    return -(-a // b)


def pass_axes(shape, dim, ori):
    return [a for a in range(3) if dim == "3D" or a != AXIS[ori]]


def test_constants_and_the_two_fit_radii(ivxlib):
    """The boundaries the cases below stand on: 224 / 225 for an int16 tile, 32 / 33 for a float64 one, and the x
    pass staged in LDS for every radius the library accepts."""
    from invesalius3_amd import filters as F
    assert F.MAX_RADIUS == MAX_RADIUS
    assert zy_tile_bytes(224, I16) == LDS_LIMIT and zy_in_lds(224, I16) and not zy_in_lds(225, I16)
    assert zy_tile_bytes(32, F64) == LDS_LIMIT and zy_in_lds(32, F64) and not zy_in_lds(33, F64)
    assert x_in_lds(MAX_RADIUS, F64)
    assert [radius(s) for s in (56.0, 56.2, 63.8, 63.9, 8.0, 8.2, 10.0)] == [224, 225, 255, 256, 32, 33, 40]


@functools.lru_cache(maxsize=None)
def _vol(shape, seed=0):
    """full-range int16 noise; shared between tests, so read-only"""
    a = np.random.default_rng(4100 + seed).integers(-32768, 32768, shape).astype(np.int16)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _strided():
    view = _vol((140, 131, 201), 7)[::2, 1:-1, ::3]
    assert view.shape == (70, 129, 67) and not view.flags["C_CONTIGUOUS"]
    return view


def _want_of(img, ft, v, dim, ori, normalize=True):
    w = _ref(ft, img, v, normalize) if dim == "3D" else _ref_2d(ft, img, v, ori, normalize)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _want(shape, ft, v, dim, ori, seed=0):
    return _want_of(_vol(shape, seed), ft, v, dim, ori)


def _same(got, want):
    return isinstance(got, np.ndarray) and got.dtype == np.int16 and got.shape == want.shape and np.array_equal(got, want)


def _check_modes(img, ft, v, modes, want_fn):
    """filters.* on the whole volume and slice_.apply_image_filter in every mode of `modes`, against want_fn(dim, ori)"""
    from invesalius3_amd import slice_
    bad = []
    for dim, ori in modes:
        want = want_fn(dim, ori)
        assert want.dtype == np.int16
        if dim == "3D" and not _same(_fn(ft)(img, v), want):
            bad.append(("filters", ft, v, dim))
        if not _same(slice_.apply_image_filter(img, ft, v, dim, ori), want):
            bad.append(("apply_image_filter", ft, v, dim, ori))
    assert not bad, bad


# -- A. the LDS-fit switch and the fallback kernel ---------------------------------------------------------------------------
LONG = 460


@pytest.mark.parametrize("ft", [0, 4])
@pytest.mark.parametrize("sigma", [56.0, 56.2, 63.8])
@pytest.mark.parametrize("shape", [(LONG, 3, 5), (3, LONG, 5)], ids=_sid)
def test_gaussian_at_the_lds_fit_switch(ivxlib, shape, sigma, ft):
    """<int16,int16>: r = 224 is the largest k_sym_zy tile (exactly 64 KB of dynamic LDS), r = 225 the first k_sym_pass,
    r = 255 the cap.  Along the long axis r = 225 has interior outputs (no reflection); the axes of 3 and 5 fold the
    reflection dozens of times.  3-D, and 2-D in the two orientations that keep the long axis as a pass axis."""
    r = radius(sigma)
    long_ax = shape.index(LONG)
    assert r <= MAX_RADIUS and x_in_lds(r, I16)
    assert zy_in_lds(r, I16) == (sigma == 56.0)
    if sigma == 56.0:
        assert zy_tile_bytes(r, I16) == LDS_LIMIT
    if sigma == 56.2:
        assert LONG > 2 * r  # c - r >= 0 && c + r < n for some c: the interior branch of k_sym_pass
    assert r >= 24 * max(s for s in shape if s != LONG)  # two dozen folds of the short axes at the least
    modes = [m for m in MODES if m[0] == "3D" or AXIS[m[1]] != long_ax]
    assert len(modes) == 3 and all(long_ax in pass_axes(shape, d, o) for d, o in modes)
    _check_modes(_vol(shape), ft, sigma, modes, lambda dim, ori: _want(shape, 0, sigma, dim, ori))


@pytest.mark.parametrize("sigma", [8.0, 8.2, 10.0])
@pytest.mark.parametrize("shape", [(70, 75, 40), (70, 20, 40)], ids=_sid)
def test_border_float64_pass_at_the_lds_fit_switch(ivxlib, shape, sigma):
    """The border pre-smoothing's first pass reads int16 (<int16,double>), every later one float64 (<double,double>).
    Only axis 1 as the SECOND pass can take <double,double> to the fallback: axis 2 is k_sym_x at any radius, and
    axis 0, when it has a pass, is always the first.  Axis 1 is second in 3-D and in 2-D Sagittal (pass axes 0, 1);
    in 2-D Axial it is first, in Coronal it has no pass.  r = 32 is the largest float64 tile (exactly 64 KB), 33 the
    first fallback; ny = 75 > 2 * 33 has interior outputs, ny = 20 sends every output to the reflecting branch."""
    r = radius(sigma)
    assert zy_in_lds(r, I16) and x_in_lds(r, F64)  # the first pass never falls back here
    assert zy_in_lds(r, F64) == (sigma == 8.0)
    if sigma == 8.0:
        assert zy_tile_bytes(r, F64) == LDS_LIMIT
    if sigma == 8.2:
        assert (shape[1] > 2 * r) == (shape[1] == 75) and (shape[1] == 75 or shape[1] <= r)
    modes = [("3D", "Axial"), ("2D", "Sagittal")]
    assert all(pass_axes(shape, d, o)[:2] == [0, 1] for d, o in modes)
    assert pass_axes(shape, "2D", "Axial")[0] == 1 and 1 not in pass_axes(shape, "2D", "Coronal")
    _check_modes(_vol(shape), 5, sigma, modes, lambda dim, ori: _want(shape, 5, sigma, dim, ori))


@pytest.mark.parametrize("shape", [(LONG, 3, 5), (3, LONG, 5)], ids=_sid)
def test_border_first_pass_in_the_fallback(ivxlib, shape):
    """sigma 56.2: <int16,double> leaves LDS too, on the first pass axis -- axis 0 in 3-D, the long axis 1 in 2-D Axial."""
    sigma = 56.2
    r = radius(sigma)
    assert not zy_in_lds(r, I16) and not zy_in_lds(r, F64) and LONG > 2 * r
    modes = [("3D", "Axial")] + ([("2D", "Axial")] if shape[1] == LONG else [])
    assert pass_axes(shape, "2D", "Axial")[0] == 1
    _check_modes(_vol(shape), 5, sigma, modes, lambda dim, ori: _want(shape, 5, sigma, dim, ori))


def test_radius_cap_raises_everywhere(ivxlib):
    """sigma 63.9 needs r = 256 > IVX_FILTER_MAX_RADIUS: ValueError from filters.*, apply_image_filter and
    DeviceVolume.filter_image, before anything is launched."""
    from invesalius3_amd import filters as F
    from invesalius3_amd import slice_
    from invesalius3_amd.device import DeviceVolume
    sigma = 63.9
    assert radius(sigma) == MAX_RADIUS + 1
    img = _vol((LONG, 3, 5))
    for fn in (F.gaussian_blur_filter, F.despeckle_filter, F.border_detection_filter):
        with pytest.raises(ValueError):
            fn(img, sigma)
    for ft in (0, 4, 5):
        for dim, ori in (("3D", "Axial"), ("2D", "Coronal")):
            with pytest.raises(ValueError):
                slice_.apply_image_filter(img, ft, sigma, dim, ori)
    vol = DeviceVolume(img)
    try:
        for ft in (0, 4, 5):
            with pytest.raises(ValueError):
                vol.filter_image(ft, sigma)
        vol.sync()
        assert np.array_equal(vol.image.download(img.shape, np.int16), img)
    finally:
        vol.close()


def test_radius_cap_in_the_library(ivxlib):
    """ivx_dev_filter_gaussian_i16 with radius 256: the invalid-argument code, and the output buffer untouched."""
    from invesalius3_amd.device import DeviceBuffer
    L = ivxlib
    lib = L.lib()
    shape = (9, 10, 11)
    img = _vol(shape)
    sentinel = np.full(shape, 12345, np.int16)
    nb = ctypes.c_size_t(0)
    L.check(lib.ivx_filter_scratch_bytes(0, L.i64(shape), -1, ctypes.byref(nb)), "filter_scratch_bytes")
    src, out, scratch = DeviceBuffer(img.nbytes), DeviceBuffer(img.nbytes), DeviceBuffer(nb.value)
    try:
        src.upload(img)
        out.upload(sentinel)
        r = MAX_RADIUS + 1
        w = np.full(2 * r + 1, 1.0 / (2 * r + 1))
        rc = lib.ivx_dev_filter_gaussian_i16(src.ptr, L.i64(shape), -1, L.ptr(w), r, out.ptr, scratch.ptr, None)
        assert rc == L.IVX_EINVAL and "radius" in L.last_error()
        L.synchronize()
        assert np.array_equal(out.download(shape, np.int16), sentinel)
        # the same call at the cap is accepted (the weights of sigma 63.8)
        from invesalius3_amd import filters as F
        w, r = F.gaussian_weights(63.8)
        assert r == MAX_RADIUS
        L.check(lib.ivx_dev_filter_gaussian_i16(src.ptr, L.i64(shape), -1, L.ptr(w), r, out.ptr, scratch.ptr, None), "gaussian")
        L.synchronize()
        assert np.array_equal(out.download(shape, np.int16), _want(shape, 0, 63.8, "3D", "Axial"))
    finally:
        for b in (src, out, scratch):
            b.close()


# -- B. more than one tile or segment ----------------------------------------------------------------------------------------
LIVE = [(0, 1.0), (0, 2.5), (1, 1.0), (1, 1.6), (1, 3.0), (2, 0.5), (2, 3.0), (3, 1.0), (4, 0.7), (5, 1.0), (5, 2.0)]
VALUES = LIVE + [(0, 10.0), (2, 15.0)]  # r = 40: wider than every tile remainder below; mean size 31
WIDE = (2, 3, 8200)

# shape -> per axis (tiles, outputs in the last tile) of LT for z and y and of XT for x
TILES = {
    (3, 5, 1061): ((1, 3), (1, 5), (2, 37)),
    (2, 3, 1025): ((1, 2), (1, 3), (2, 1)),
    (2, 3, 2049): ((1, 2), (1, 3), (3, 1)),
    (70, 129, 67): ((2, 6), (3, 1), (1, 67)),
    (129, 3, 5): ((3, 1), (1, 3), (1, 5)),
    (3, 65, 5): ((1, 3), (2, 1), (1, 5)),
    WIDE: ((1, 2), (1, 3), (9, 8)),
}


def _assert_tiling(shape):
    for n, t, (tiles, last) in zip(shape, (LT, LT, XT), TILES[shape]):
        assert (cdiv(n, t), n - (cdiv(n, t) - 1) * t) == (tiles, last)
    assert LT == BOX_SEG  # so a partial k_sym_zy tile is a partial k_box_pass segment too
    assert any(tiles > 1 for tiles, _ in TILES[shape])
    r = radius(10.0)
    for ax, (tiles, last) in enumerate(TILES[shape]):
        if tiles > 1:  # the halo of the last tile folds over all of it into its neighbour; along z / y so does the size-31 box
            assert last < r and (ax == 2 or last < 31)
    if shape[2] > XT:
        assert shape[2] > MINMAX_STRIDE
    if shape == (3, 5, 1061):
        assert cdiv(shape[2], 32) == 34  # x tiles of k_median and k_sobel_mag
    if shape == (70, 129, 67):
        assert cdiv(shape[2], LANES) == 2 and shape[2] - LANES == 3  # the second x block of k_sym_zy has nxb = 3
        assert cdiv(shape[0] * shape[1], max(MINMAX_ROW_BUDGET // shape[2], 64)) > 1  # k_seg_minmax_x: several row chunks
        assert 70 <= cdiv(shape[0] * shape[1], MINMAX_ROW_BUDGET // shape[2]) <= 80  # k_seg_minmax_rows, 3-D
    if shape == WIDE:
        assert MINMAX_ROW_BUDGET // shape[2] == 0  # rpb = max(1, 0) = 1


@pytest.mark.parametrize("ft,v", VALUES)
@pytest.mark.parametrize("shape", [s for s in TILES if s != WIDE], ids=_sid)
def test_past_one_tile(ivxlib, shape, ft, v):
    """All six filters, 3-D and the three 2-D orientations, on shapes with two or three k_sym_x row tiles (last one of
    37 or 1), k_sym_zy tiles and box segments with a last one of 6 or 1 (shorter than r = 40 and than the size-31 box),
    a second x block of 3 lanes, rows wider than 256 for the min / max kernels."""
    _assert_tiling(shape)
    _check_modes(_vol(shape), ft, v, MODES, lambda dim, ori: _want(shape, ft, v, dim, ori))


@pytest.mark.parametrize("ft,v", [(ft, v) for ft, v in VALUES if ft in (0, 3, 5)])
def test_row_wider_than_the_minmax_budget(ivxlib, ft, v):
    """nx = 8200 > 8192: rpb = 1 in seg_minmax(), nine k_sym_x tiles.  Gaussian, sharpen and border."""
    _assert_tiling(WIDE)
    _check_modes(_vol(WIDE), ft, v, MODES, lambda dim, ori: _want(WIDE, ft, v, dim, ori))


@pytest.mark.parametrize("ft,v", VALUES)
def test_past_one_tile_strided_view(ivxlib, ft, v):
    """a stepped, non-contiguous view that lands on (70, 129, 67): the strided upload feeds the same tiles"""
    view = _strided()
    _assert_tiling(view.shape)
    got = _fn(ft)(view, v)
    assert got.flags["C_CONTIGUOUS"] and _same(got, _ref(ft, np.ascontiguousarray(view), v))


# -- C. degenerate sigma, int16's ends, flat slices ------------------------------------------------------------------------
@pytest.mark.parametrize("ft", [0, 4, 5])
@pytest.mark.parametrize("sigma", [0.0, 1e-16])
def test_sigma_too_small_for_a_pass(ivxlib, sigma, ft):
    """sigma <= 1e-15: scipy's gaussian_filter skips every axis.  radius < 0 in the library: a device copy for Gaussian
    and despeckle (the input comes back), k_widen and then Sobel for border."""
    from invesalius3_amd import filters as F
    assert F.gaussian_weights(sigma) == (None, -1)
    shape = (19, 33, 41)
    img = _vol(shape)
    modes = [("3D", "Axial"), ("2D", "Axial")]
    _check_modes(img, ft, sigma, modes, lambda dim, ori: _want(shape, ft, sigma, dim, ori))
    if ft != 5:
        for dim, ori in modes:
            assert np.array_equal(_want(shape, ft, sigma, dim, ori), img)


@functools.lru_cache(maxsize=None)
def _extreme(name):
    if name == "checkerboard":
        z, y, x = np.indices((9, 10, 11))
        a = np.where((z + y + x) % 2 == 0, -32768, 32767).astype(np.int16)
    else:
        a = _vol((19, 33, 41)).copy()
        a[0, 0, 0], a[-1, -1, -1], a[9, 16, 20], a[9, 16, 21] = -32768, 32767, 32767, -32768
    assert a.min() == -32768 and a.max() == 32767
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("ft,v", LIVE + [(3, 0.3), (3, 4.7)])
@pytest.mark.parametrize("name", ["checkerboard", "noise"])
def test_int16_extremes(ivxlib, name, ft, v):
    """-32768 and 32767 in the input: the median's bit search over a 65535-wide range, the box sums, sharpen's clip at
    the type's limits, border's rescale with a span of 65535."""
    img = _extreme(name)
    _check_modes(img, ft, v, MODES, lambda dim, ori: _want_of(img, ft, v, dim, ori))


@pytest.mark.parametrize("v", [1.0, 2.0])
@pytest.mark.parametrize("name", ["checkerboard", "noise"])
def test_int16_extremes_border_without_normalize(ivxlib, name, v):
    from invesalius3_amd import filters as F
    img = _extreme(name)
    assert _same(F.border_detection_filter(img, v, normalize=False), _ref(5, img, v, normalize=False))
    for k in (0, img.shape[0] - 1):  # a 2-D image
        assert _same(F.border_detection_filter(img[k], v, normalize=False), _ref(5, img[k], v, normalize=False))


@pytest.mark.parametrize("ft,v", [(3, 1.0), (3, 4.7), (5, 1.0)])
def test_some_slices_flat(ivxlib, ft, v):
    """One constant axial, coronal and sagittal slice in a full-range volume: in the 2-D run of that orientation the clip
    range and the `range > 0` decision of the border rescale differ from slice to slice."""
    img = _vol((6, 7, 8), 3).copy()
    img[2], img[:, 3], img[:, :, 5] = 117, 117, 117
    for ax in range(3):
        flat = [k for k in range(img.shape[ax]) if np.ptp(np.take(img, k, axis=ax)) == 0]
        assert len(flat) == 1
    _check_modes(img, ft, v, MODES, lambda dim, ori: _want_of(img, ft, v, dim, ori))
    if ft == 5:  # what the flat slice must come out as: no gradient, not rescaled
        for ori, sl in (("Axial", np.s_[2]), ("Coronal", np.s_[:, 3]), ("Sagittal", np.s_[:, :, 5])):
            assert not _ref_2d(ft, img, v, ori)[sl].any()


# -- D. the resident path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ft,v,dim,ori", [((70, 75, 40), 5, 8.2, "3D", "Axial"), ((LONG, 3, 5), 0, 56.2, "3D", "Axial"),
                                                ((70, 129, 67), 2, 15.0, "2D", "Coronal")],
                         ids=["border-double-fallback", "gaussian-int16-fallback", "mean-partial-segment"])
def test_device_volume_filter_at_the_edges(ivxlib, shape, ft, v, dim, ori):
    """DeviceVolume.filter_image == slice_.apply_image_filter on the host array == scipy: the <double,double> fallback,
    the <int16,int16> fallback, and box segments past the first with a partial last one."""
    from invesalius3_amd import slice_
    from invesalius3_amd.device import DeviceVolume
    if ft == 5:
        assert not zy_in_lds(radius(v), F64) and pass_axes(shape, dim, ori)[1] == 1
    elif ft == 0:
        assert not zy_in_lds(radius(v), I16) and shape[0] > 2 * radius(v)
    else:
        assert int(2 * v + 1) == 31 and pass_axes(shape, dim, ori) == [0, 2] and 0 < shape[0] - BOX_SEG < 31
    img = _vol(shape)
    want = _want(shape, 0 if ft == 4 else ft, v, dim, ori)
    host = slice_.apply_image_filter(img, ft, v, dim, ori)
    assert _same(host, want)
    vol = DeviceVolume(img)
    try:
        vol.filter_image(ft, v, dim, ori)
        vol.sync()
        assert _same(vol.image.download(img.shape, np.int16), host)
    finally:
        vol.close()
