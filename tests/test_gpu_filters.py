"""Image filters (k_filter.hip) bit for bit: the reference's own dispatch results (tests/golden/ref_filters.npz), live
scipy.ndimage on synthetic volumes (odd, even, strided, whole-volume sizes), and the resident DeviceVolume.filter_image
feeding threshold / region growing."""
import functools
import os
import time

import numpy as np
import pytest
import scipy.ndimage as ndi

from _filters_ref import AXIS, _fn, _ref, _ref_2d
from conftest import synth_volume

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_filters.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    cases = []
    for i, name in enumerate(g["case_names"]):
        vn, ft, v, dim, ori = str(name).split("|")
        cases.append((i, vn, int(ft), float(v), dim, ori))
    return g, cases


@pytest.mark.parametrize("ft", range(6))
def test_golden_dispatch(ivxlib, golden, ft):
    """slice_.apply_image_filter == the reference's _run_filter, 3-D and 2-D in every orientation (one call each)."""
    from invesalius3_amd import slice_
    g, cases = golden
    bad = []
    n = 0
    for i, vn, t, v, dim, ori in cases:
        if t != ft:
            continue
        got = slice_.apply_image_filter(g["vol_" + vn], ft, v, dim, ori)
        n += 1
        if got.dtype != np.int16 or not np.array_equal(got, g["out_%d" % i]):
            bad.append((vn, v, dim, ori))
    assert n > 0 and not bad, bad


@pytest.mark.parametrize("ft", range(6))
def test_golden_functions_and_slices(ivxlib, golden, ft):
    """filters.* on the whole volume (3-D cases) and, for the 2-D cases, on every slice view m[i], m[:, i], m[:, :, i]
    (strided 2-D arrays) -- the reference's own slice loop."""
    g, cases = golden
    fn = _fn(ft)
    bad = []
    for i, vn, t, v, dim, ori in cases:
        if t != ft:
            continue
        vol, want = g["vol_" + vn], g["out_%d" % i]
        if dim == "3D":
            if not np.array_equal(fn(vol, v), want):
                bad.append((vn, v, dim))
            continue
        ax = AXIS[ori]
        for k in range(vol.shape[ax]):
            sl = (slice(None),) * ax + (k,)
            if not np.array_equal(fn(vol[sl], v), want[sl]):
                bad.append((vn, v, ori, k))
                break
    assert not bad, bad


def test_golden_border_no_normalize_and_2d_image(ivxlib, golden):
    from invesalius3_amd import filters as F
    g, _ = golden
    for key in g.files:
        if key.startswith("nonorm_"):
            _, vn, v = key.split("_")
            assert np.array_equal(F.border_detection_filter(g["vol_" + vn], float(v), normalize=False), g[key]), key
        elif key.startswith("img2d_"):
            _, ft, v = key.split("_")
            assert np.array_equal(_fn(int(ft))(g["img2d"], float(v)), g[key]), key


# -- live scipy, the reference's formulas restated on scipy (filters.py:5-66; _ref and _ref_2d of _filters_ref.py) ------
LIVE = [(0, 1.0), (0, 2.5), (1, 1.0), (1, 1.6), (1, 3.0), (2, 0.5), (2, 3.0), (3, 1.0), (4, 0.7), (5, 1.0), (5, 2.0)]


@pytest.mark.parametrize("shape", [(19, 33, 41), (24, 32, 48)])
@pytest.mark.parametrize("ft,v", LIVE)
def test_live_scipy_3d(ivxlib, shape, ft, v):
    img = synth_volume(shape, seed=5 + ft)
    assert np.array_equal(_fn(ft)(img, v), _ref(ft, img, v))


@pytest.mark.parametrize("ft,v", LIVE)
def test_live_scipy_strided_view(ivxlib, ft, v):
    base = synth_volume((30, 41, 50), seed=11)
    view = base[2::2, 1:-3, ::3]
    assert not view.flags["C_CONTIGUOUS"]
    got = _fn(ft)(view, v)
    assert got.flags["C_CONTIGUOUS"] and np.array_equal(got, _ref(ft, np.ascontiguousarray(view), v))


@pytest.mark.parametrize("ft,v", [(0, 1.5), (1, 2.0), (2, 2.0), (3, 2.0), (5, 1.0)])
@pytest.mark.parametrize("ori", ["Axial", "Coronal", "Sagittal"])
def test_live_scipy_2d_mode(ivxlib, ft, v, ori):
    """apply_image_filter's 2-D mode == the reference's slice loop with live scipy on each slice."""
    from invesalius3_amd import slice_
    img = synth_volume((12, 17, 22), seed=3)
    assert np.array_equal(slice_.apply_image_filter(img, ft, v, "2D", ori), _ref_2d(ft, img, v, ori))


def test_border_magnitude_over_int16_no_normalize(ivxlib):
    """|grad| > 32767: astype(int16) wraps (int32 truncation, low 16 bits), as numpy does on x86-64."""
    from invesalius3_amd import filters as F
    img = np.zeros((10, 12, 14), np.int16)
    img[:, :, 7:] = 30000
    img[:5, :6, :3] = -30000
    mag = _ref(5, img, 0.1, normalize=False)
    f = ndi.gaussian_filter(img.astype(float), sigma=0.1)
    assert np.sqrt(sum(ndi.sobel(f, axis=a) ** 2 for a in range(3))).max() > 32767
    assert np.array_equal(F.border_detection_filter(img, 0.1, normalize=False), mag)


@pytest.mark.parametrize("ft,v,n", [(0, 1.0, 512), (2, 3.0, 512), (1, 2.0, 192)])
def test_whole_volume_sizes(ivxlib, ft, v, n):
    """Gaussian sigma 1 and mean size 7 at 512^3, median 5^3 at 192^3, against scipy on the same call."""
    img = synth_volume((n, n, n), seed=21) if n <= 192 else _big(n)
    t0 = time.perf_counter()
    want = _ref(ft, img, v)
    t_cpu = time.perf_counter() - t0
    got = _fn(ft)(img, v)
    assert np.array_equal(got, want), (ft, v, n, t_cpu)


@functools.lru_cache(maxsize=1)
def _big(n):
    """a 512^3 CT-like volume made quickly: a smooth field plus hashed noise (synth_volume's meshgrid is slow here)"""
    z = np.linspace(0, 1, n)[:, None, None]
    y = np.linspace(0, 1, n)[None, :, None]
    x = np.linspace(0, 1, n)[None, None, :]
    f = 1500.0 * np.exp(-((z - 0.5) ** 2 + (y - 0.45) ** 2 + (x - 0.55) ** 2) / 0.05) + 150.0 * np.sin(6.0 * x + 2.0 * y) * np.cos(5.0 * z)
    f = f - 900.0 + np.random.default_rng(3).integers(-60, 61, (n, n, n))
    return np.clip(f, -1024, 3071).astype(np.int16)


# -- the resident volume ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft,v,dim,ori", [(1, 1.0, "3D", "Axial"), (0, 2.0, "3D", "Axial"), (2, 1.0, "2D", "Coronal"),
                                          (3, 2.0, "3D", "Axial"), (5, 1.0, "2D", "Sagittal")])
def test_device_volume_filter_then_threshold_and_grow(ivxlib, ft, v, dim, ori):
    from invesalius3_amd import invesalius_rs as rs
    from invesalius3_amd import slice_
    from invesalius3_amd.device import DeviceVolume
    img = synth_volume((40, 48, 64), seed=9)
    host = slice_.apply_image_filter(img, ft, v, dim, ori)
    vol = DeviceVolume(img)
    try:
        lo, hi = 150, 3071
        vol.threshold(lo, hi)  # derived state made from the unfiltered image first ...
        vol.filter_image(ft, v, dim, ori)  # ... must be dropped
        vol.sync()
        assert np.array_equal(vol.image.download(img.shape, np.int16), host)
        vol.threshold(lo, hi)
        m = np.zeros(tuple(s + 1 for s in img.shape), np.uint8)
        slice_.do_threshold_to_all_slices(m, host, (lo, hi))
        assert np.array_equal(vol.download_mask(), m[1:, 1:, 1:])
        z, y, x = (int(c[len(c) // 2]) for c in np.nonzero((host >= lo) & (host <= hi)))
        strct = np.ones((3, 3, 3), np.uint8)
        vol.zero_out_mask()
        vol.region_grow([(x, y, z)], lo, hi, strct, fill=1, select_value=None)
        want = np.zeros(img.shape, np.uint8)
        rs.floodfill_threshold(host, [(x, y, z)], lo, hi, 1, strct, want)
        assert np.array_equal(vol.download_out_mask(), want)
    finally:
        vol.close()
