"""GPU: volume rendering (csrc/k_volren.hip through DeviceVolume.render_volume / volume_histogram and the host entry)
against the float64 restatement of the contract in tests/_volren_ref.py, with the reference's 30 presets from
tests/golden/ref_volume.npz."""
import numpy as np
import pytest

import _volren_ref as R

pytestmark = pytest.mark.gpu

PRESETS, CLUTS, _ = R.fixture()
NAMES = sorted(PRESETS)
SHAPE, SPACING, SIZE = (34, 40, 44), (0.9, 0.7, 1.3), (48, 40)
TOL = 1e-3
_IMG = R.synth_volume(SHAPE, seed=5)
_FIELDS = {}
MAX_ERR = []


def _field(img, setup):
    key = (id(img), setup["shift"], len(setup["kernels"]))
    if key not in _FIELDS:
        _FIELDS[key] = R.prepare(img, setup["shift"], setup["kernels"])
    return _FIELDS[key]


def _oracle(img, spacing, preset, view, size, **kw):
    from invesalius3_amd import volume as V
    cam = V.camera_for_view(view, img.shape, spacing, size) if isinstance(view, str) else view
    setup = V.render_setup(preset, (int(img.min()), int(img.max())), cam, color_lists=CLUTS, **kw)
    return R.render(_field(img, setup), spacing, setup)


@pytest.fixture(scope="module")
def dvol(ivxlib):
    from invesalius3_amd.device import DeviceVolume
    v = DeviceVolume(_IMG, spacing=SPACING)
    yield v
    v.close()


def _check(got, ref, frac=0.0):
    err = np.abs(got.astype(np.float64) - ref)
    MAX_ERR.append(float(err.max()))
    bad = np.count_nonzero(err.max(-1) > TOL)
    assert bad <= frac * err.shape[0] * err.shape[1], "max error %.3g, %d pixels over %g" % (err.max(), bad, TOL)


@pytest.mark.parametrize("nsmooth", [0, 1, 2])
def test_prepare_bit_exact(ivxlib, nsmooth):
    from invesalius3_amd import volume as V
    from invesalius3_amd.device import DeviceVolume
    w = V.convolution_kernels({"convolutionFilters": ["Basic Smooth 5x5"] * nsmooth})
    # a synth volume, and constant 5x5 plates of many values (the v - 1 truncation cases)
    vals = np.arange(-32768, 32768, 37, dtype=np.int64)
    plates = np.repeat(vals[:, None, None], 6, 1).repeat(7, 2).astype(np.int16)
    pos = (_IMG.astype(np.int32) + 1100).astype(np.int16)  # min 76 > 0: the shift is +76 (the shift quirk)
    for img, shift in ((_IMG, 1024), (plates, 32768), (pos, 76)):
        with DeviceVolume(img) as v:
            vr = v._volren_field(shift, w)
            v.sync()
            got = vr["vol"].download(img.shape, np.uint16)
            cells = vr["cells"].download(tuple(vr["cshape"]) + (2,), np.uint16)
        ref = R.prepare(img, shift, w)
        assert np.array_equal(got, ref)
        assert np.array_equal(cells, R.cells(ref))
    if nsmooth:
        low = R.prepare(plates, 32768, w)[:, 3, 3].astype(np.int64) < vals + 32768
        assert low.any()  # the truncation cases are in there


@pytest.mark.parametrize("view", ["front", "iso"])
@pytest.mark.parametrize("name", NAMES)
def test_all_presets(dvol, name, view):
    got = dvol.render_volume(PRESETS[name], view, SIZE, color_lists=CLUTS)
    ref = _oracle(_IMG, SPACING, PRESETS[name], view, SIZE)
    assert got.shape == (SIZE[1], SIZE[0], 4) and got.dtype == np.float32
    _check(got, ref)
    if view == "iso" and not PRESETS[name].get("MIP"):
        assert np.count_nonzero(got[..., 3] > 0.01) > 20  # something is drawn


@pytest.mark.parametrize("shade", [True, False])
@pytest.mark.parametrize("name", ["Bone + Skin", "Gold Bone", "Standard", "Vascular", "Pencil"])
def test_shaded_unshaded(dvol, name, shade):
    got = dvol.render_volume(PRESETS[name], "iso", SIZE, shade=shade, color_lists=CLUTS)
    _check(got, _oracle(_IMG, SPACING, PRESETS[name], "iso", SIZE, shade=shade))


@pytest.mark.parametrize("view", ["front", "back", "left", "right", "top", "bottom", "iso"])
def test_all_views(dvol, view):
    got = dvol.render_volume(PRESETS["Soft + Skin"], view, SIZE, shade=True, color_lists=CLUTS)
    _check(got, _oracle(_IMG, SPACING, PRESETS["Soft + Skin"], view, SIZE, shade=True))


@pytest.mark.parametrize("name", ["Bone + Skin", "Standard", "MIP"])
def test_cut_plane(dvol, name):
    from invesalius3_amd import volume as V
    b = V.volume_bounds(SHAPE, SPACING)
    o = np.array([(b[0] + b[1]) / 2, (b[2] + b[3]) / 2, (b[4] + b[5]) / 2])
    n = np.array([1.0, -0.4, 0.3]) / np.linalg.norm([1.0, -0.4, 0.3])
    got = dvol.render_volume(PRESETS[name], "iso", SIZE, clip_plane=(n, o), color_lists=CLUTS)
    ref = _oracle(_IMG, SPACING, PRESETS[name], "iso", SIZE, clip_plane=(n, o))
    _check(got, ref, frac=0.001)
    full = dvol.render_volume(PRESETS[name], "iso", SIZE, color_lists=CLUTS)
    assert not np.array_equal(got, full)


def test_wwwl_rerender_equals_fresh(dvol, ivxlib):
    from invesalius3_amd import volume as V
    from invesalius3_amd.device import DeviceVolume
    for name, ww, wl in (("Bone + Skin", 300.0, 200.0), ("Standard", 500.0, 100.0)):
        dvol.render_volume(PRESETS[name], "iso", SIZE, color_lists=CLUTS)
        p2 = V.set_wwwl(PRESETS[name], ww, wl, 0)
        again = dvol.render_volume(p2, "iso", SIZE, color_lists=CLUTS)
        with DeviceVolume(_IMG, spacing=SPACING) as v:
            fresh = v.render_volume(p2, "iso", SIZE, color_lists=CLUTS)
        assert np.array_equal(again, fresh)
        _check(again, _oracle(_IMG, SPACING, p2, "iso", SIZE))


def test_skipping_changes_no_bit(dvol, monkeypatch):
    skipped = 0
    for name in NAMES:
        for shade in (None, True):
            on = dvol.render_volume(PRESETS[name], "iso", SIZE, shade=shade, color_lists=CLUTS)
            st = dict(dvol.last_render_stats)
            on2 = dvol.render_volume(PRESETS[name], "iso", SIZE, shade=shade, color_lists=CLUTS)
            monkeypatch.setenv("IVX_VR_SKIP", "0")
            off = dvol.render_volume(PRESETS[name], "iso", SIZE, shade=shade, color_lists=CLUTS)
            assert dvol.last_render_stats["skipped"] == 0
            monkeypatch.delenv("IVX_VR_SKIP")
            assert np.array_equal(on.view(np.uint32), off.view(np.uint32)), name
            assert np.array_equal(on.view(np.uint32), on2.view(np.uint32)), name
            skipped += st["skipped"]
    assert skipped > 0


def test_histogram(dvol, ivxlib):
    from invesalius3_amd import volume as V
    from invesalius3_amd.device import DeviceVolume
    h = dvol.volume_histogram()
    lo, hi = int(_IMG.min()), int(_IMG.max())
    v = _IMG.ravel().astype(np.int64) - lo
    assert h.dtype == np.uint64 and np.array_equal(h, np.bincount(v[v < hi - lo], minlength=hi - lo))
    assert np.array_equal(h, V.calculate_histogram(_IMG))
    wide = np.random.default_rng(1).integers(-32768, 32767, (8, 30, 40)).astype(np.int16)  # > 16384 bins: global path
    with DeviceVolume(wide) as w:
        assert np.array_equal(w.volume_histogram(), V.calculate_histogram(wide))
    with DeviceVolume(np.full((3, 4, 5), 9, np.int16)) as c:
        assert len(c.volume_histogram()) == 0


def test_render_after_filter(ivxlib):
    from invesalius3_amd import filters
    from invesalius3_amd.device import DeviceVolume
    with DeviceVolume(_IMG, spacing=SPACING) as v:
        before = v.render_volume(PRESETS["Bone + Skin"], "iso", SIZE, color_lists=CLUTS)
        v.filter_image(filters.MEDIAN, 3.0)
        v.sync()
        filt = v.image.download(SHAPE, np.int16)
        after = v.render_volume(PRESETS["Bone + Skin"], "iso", SIZE, color_lists=CLUTS)
    assert not np.array_equal(before, after)
    _check(after, _oracle(filt, SPACING, PRESETS["Bone + Skin"], "iso", SIZE))


def test_host_entry_and_rgba8(dvol):
    from invesalius3_amd import volume as V
    for name in ("Gold Bone", "MIP", "Standard"):
        dev = dvol.render_volume(PRESETS[name], "front", SIZE, color_lists=CLUTS)
        host = V.volume_render(_IMG, SPACING, PRESETS[name], "front", SIZE, color_lists=CLUTS)
        assert np.array_equal(dev, host)
        u8 = dvol.render_volume(PRESETS[name], "front", SIZE, color_lists=CLUTS, rgba8=True)
        assert u8.dtype == np.uint8 and np.abs(u8.astype(int) - V.to_rgba8(dev).astype(int)).max() <= 1


def test_large_volume_strided_pixels(ivxlib):
    """one 512^3 render at 1024^2 against the oracle on a strided subset of the pixels"""
    from invesalius3_amd import volume as V
    from invesalius3_amd.device import DeviceVolume
    n = 512
    z = np.arange(n, dtype=np.float32)[:, None, None]
    y = np.arange(n, dtype=np.float32)[None, :, None]
    x = np.arange(n, dtype=np.float32)[None, None, :]
    r2 = (z - 256) ** 2 + (y - 250) ** 2 + (x - 262) ** 2
    img = np.full((n, n, n), -1024, np.int16)
    img[(r2 < 200.0 ** 2)] = 40
    img[(r2 < 150.0 ** 2) & (r2 > 120.0 ** 2)] = 700
    img[((z - 200) ** 2 + (y - 300) ** 2 + (x - 220) ** 2) < 40.0 ** 2] = 1500
    del r2
    img[100:110, 100:400, 120:380] = 300
    img[n // 2, n // 2, n // 2] = 3071
    spacing, size = (0.5, 0.5, 0.6), (1024, 1024)
    preset = PRESETS["Standard"]
    with DeviceVolume(img, spacing=spacing) as v:
        got = v.render_volume(preset, "iso", size, color_lists=CLUTS)
    rows, cols = np.meshgrid(np.arange(3, 1024, 16), np.arange(5, 1024, 16), indexing="ij")
    cam = V.camera_for_view("iso", img.shape, spacing, size)
    setup = V.render_setup(preset, (int(img.min()), int(img.max())), cam, color_lists=CLUTS)
    ref = R.render(R.prepare(img, setup["shift"], setup["kernels"]), spacing, setup, pixels=(rows.ravel(), cols.ravel()))
    g = got[rows.ravel(), cols.ravel()]
    err = np.abs(g.astype(np.float64) - ref)
    MAX_ERR.append(float(err.max()))
    assert np.count_nonzero(err.max(-1) > TOL) <= 0.001 * len(ref), err.max()
    assert np.count_nonzero(ref[:, 3] > 0.5) > 100


def test_report_max_error():
    """(runs last in this file) the largest per-channel difference seen against the oracle"""
    if MAX_ERR:
        print("volume render: max |GPU - oracle| = %.3g over %d renders" % (max(MAX_ERR), len(MAX_ERR)))
