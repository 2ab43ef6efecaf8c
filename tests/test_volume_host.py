"""CPU: the volume renderer's host side (invesalius3_amd/volume.py) against the reference's own transfer-function calls
(tests/golden/ref_volume.npz, made by make_golden_ref_volume.py) and the render oracle against closed forms."""
import json
import os
import plistlib

import numpy as np
import pytest

from invesalius3_amd import volume as V

import _volren_ref as R

PRESETS, CLUTS, NPZ = R.fixture()
NAMES = json.loads(str(NPZ["names_json"]))
META = json.loads(str(NPZ["meta_json"]))
SCALES = [tuple(int(v) for v in s) for s in NPZ["scales"]]


def _replay(calls, kind):
    """the recorded VTK calls through the VTK node rules"""
    n = V.Nodes()
    for c in calls:
        if kind == "ctf":
            n.add(c[0], c[1], c[2], c[3])
        elif c[0] == 1.0:
            n.add_segment(c[1], c[2], c[3], c[4])
        else:
            n.add(c[1], c[2])
    return n.array()


def test_fixture_covers_all_presets():
    assert len(NAMES) == 30 and len(PRESETS) == 30
    assert sum(1 for p in PRESETS.values() if p["advancedCLUT"]) == 13
    assert set(CLUTS) == {"Stern", "VR Bones", "VR Muscles-Bones", "VR Red Vessels"}


@pytest.mark.parametrize("j", range(3))
@pytest.mark.parametrize("i", range(30))
def test_nodes_equal_reference_calls(i, j):
    name, scale = NAMES[i], SCALES[j]
    p = PRESETS[name]
    got_c = V.color_nodes(p, scale, CLUTS).array()
    got_o = V.opacity_nodes(p, scale).array()
    assert np.array_equal(got_c, _replay(NPZ["%d_%d_ctf" % (i, j)], "ctf"))
    assert np.array_equal(got_o, _replay(NPZ["%d_%d_pwf" % (i, j)], "pwf"))
    m = META["%d_%d" % (i, j)]
    # shift, kernels, sample distances
    assert [a[0] for a in m["shift"]] == [float(V.shift_for(scale))]
    ks = V.convolution_kernels(p)
    assert len(ks) == len(m["kernels"]) and all(np.array_equal(k, np.array(r)) for k, r in zip(ks, m["kernels"]))
    assert ["SetImageSampleDistance", [0.25]] in m["sample"] and ["SetSampleDistance", [V.SAMPLE_DISTANCE]] in m["sample"]
    assert ["SetScalarOpacityUnitDistance", [V.OPACITY_UNIT_DISTANCE]] in m["sample"]
    # shading: the preset switch follows useShading, the first load ends in ShadeOn
    for calls, shade in ((m["prop_switch"], None), (m["prop_first"], True)):
        s = V.shading(p, shade)
        on = [c[0] for c in calls if c[0] in ("ShadeOn", "ShadeOff")][-1] == "ShadeOn"
        assert on == s["shade"]
        vals = {c[0]: c[1][0] for c in calls if c[0].startswith("Set") and c[1]}
        assert (vals["SetAmbient"], vals["SetDiffuse"], vals["SetSpecular"], vals["SetSpecularPower"]) == (
            s["ambient"], s["diffuse"], s["specular"], s["specular_power"])
    assert V.shading(p, True)["shade"] and [c[0] for c in m["prop_first"]][-1] == "ShadeOn"
    blend = "SetBlendModeToMaximumIntensity" if V.is_mip(p) else "SetBlendModeToComposite"
    assert m["mapper_first"] == [[blend, []]] and m["mapper_switch"] == [[blend, []]]


def test_wwwl_equals_reference():
    for rec in json.loads(str(NPZ["wwwl_json"])):
        p = PRESETS[rec["preset"]]
        before = json.dumps(p, sort_keys=True)
        got = V.set_wwwl(p, rec["ww"], rec["wl"], rec["curve"])
        assert json.dumps(p, sort_keys=True) == before  # the caller's preset is left alone
        assert json.dumps(got, sort_keys=True) == json.dumps(rec["after"], sort_keys=True), rec["preset"]
        if "calc" in rec:
            if rec["calc"] == "IndexError":
                with pytest.raises(IndexError):
                    V.calculate_wwwl(p, rec["curve"])
            else:
                ww, wl = V.calculate_wwwl(p, rec["curve"])
                assert (ww, wl) == tuple(rec["calc"][:2])


def test_baked_table_equals_node_evaluation():
    for name in ("Bone + Skin", "Standard", "MIP", "Pencil"):
        p = PRESETS[name]
        cn, on = V.color_nodes(p, (-1024, 3071), CLUTS), V.opacity_nodes(p, (-1024, 3071))
        rgba, a, prefix = V.bake_table(cn, on, 4095)
        q = np.arange(4097, dtype=np.float64)
        assert rgba.shape == (4097, 4) and a.shape == (4097,) and prefix.shape == (4098,)
        assert np.array_equal(rgba[:, :3], np.clip(cn.evaluate(q), 0, 1))
        assert np.array_equal(a, np.clip(on.evaluate(q)[:, 0], 0, 1))
        assert np.array_equal(rgba[:, 3], 1 - (1 - a) ** (0.4 / 2.0))
        assert np.array_equal(prefix[1:], np.cumsum(rgba[:, 3] > 0))
        # direct evaluation at a node and halfway between two nodes
        xs = on.array()
        k = int(np.argmax((xs[:, 0] > 10) & (xs[:, 0] < 4000)))
        x0 = xs[k, 0]
        if float(x0).is_integer():
            assert a[int(x0)] == xs[k, 1]


def test_node_rules():
    n = V.Nodes()
    n.add_segment(0, 0, 65535, 0)
    assert n.array().tolist() == [[0, 0], [65535, 0]]
    n.add(10, 0.5)
    n.add(5, 0.25)
    n.add(10, 0.75)  # replaces
    assert n.array().tolist() == [[0, 0], [5, 0.25], [10, 0.75], [65535, 0]]
    assert n.evaluate([7.5])[0, 0] == 0.5
    c = V.Nodes()
    c.add(100, 0.2, 0.4, 0.6)
    c.add(200, 1.0, 1.0, 1.0)
    assert np.array_equal(c.evaluate([0, 300]), [[0.2, 0.4, 0.6], [1, 1, 1]])  # clamped to the end nodes


def test_preset_loading(tmp_path):
    p = PRESETS["Bone + Skin"]
    path = tmp_path / "Bone + Skin.plist"
    with open(path, "wb") as f:
        plistlib.dump(p, f, fmt=plistlib.FMT_XML)
    a = V.load_preset(p)
    assert a == p and a is not p
    assert V.load_preset(str(path)) == p
    assert V.load_preset("Bone + Skin", str(tmp_path)) == p
    with pytest.raises(FileNotFoundError):
        V.load_preset("Nope", str(tmp_path))
    with pytest.raises(FileNotFoundError):
        V.load_preset("Bone + Skin")


def test_refusals(tmp_path):
    p = dict(PRESETS["Standard"])
    with pytest.raises(KeyError):
        V.color_nodes(dict(p, CLUT="No Such CLUT"), (-1024, 3071), CLUTS)
    os.makedirs(tmp_path / "color_list")
    with pytest.raises(FileNotFoundError):
        V.color_nodes(p, (-1024, 3071), str(tmp_path))
    with pytest.raises(KeyError):
        V.color_nodes(p, (-1024, 3071), None)
    with pytest.raises(ValueError):
        V.camera_for_view("iso", (10, 10, 10), (1, 1, 1), (0, 10))
    with pytest.raises(ValueError):
        V.camera_for_view("diagonal", (10, 10, 10), (1, 1, 1), (10, 10))
    with pytest.raises(ValueError):
        V.convolution_kernels(dict(p, convolutionFilters=["Sharpen 3x3"]))


def test_histogram_quirks():
    img = np.array([[[-3, -3, 0, 5, 5, 2]]], np.int16)
    h = V.calculate_histogram(img)
    assert len(h) == 8 and h.dtype == np.uint64
    assert h[0] == 2 and h[3] == 1 and h[5] == 1 and h.sum() == 4  # the two voxels at max are not counted
    assert len(V.calculate_histogram(np.full((2, 2, 2), 7, np.int16))) == 0


@pytest.mark.parametrize("view", sorted(V.VIEWS))
@pytest.mark.parametrize("viewport", [(64, 48), (640, 480), (300, 700)])
def test_camera_fits_the_box(view, viewport):
    shape, spacing = (40, 50, 60), (0.7, 0.8, 1.5)
    cam = V.camera_for_view(view, shape, spacing, viewport)
    d, r, u = cam["dir"], cam["right"], cam["up"]
    assert abs(np.linalg.norm(d) - 1) < 1e-12 and abs(r @ d) < 1e-12 and abs(u @ d) < 1e-12 and abs(r @ u) < 1e-12
    b = V.volume_bounds(shape, spacing)
    corners = np.array([[x, y, z] for x in b[:2] for y in b[2:4] for z in b[4:]])
    rel = corners - cam["focal"]
    w, h = viewport
    half_h = cam["parallel_scale"]
    half_w = half_h * w / h
    su, sv = np.abs(rel @ r), np.abs(rel @ u)
    assert su.max() <= half_w * (1 + 1e-9) and sv.max() <= half_h * (1 + 1e-9)  # the box projects inside the viewport
    # ... with at least the reference's smallest margin (1.15) along the tighter of the two axes for the axis views
    if view != "iso":
        assert max(su.max() / half_w, sv.max() / half_h) <= 1 / 1.15 + 1e-9
    assert (cam["position"] - cam["focal"]) @ d < 0  # the camera looks at the focal point


def test_oracle_uniform_slab_closed_form():
    """a uniform slab along the view direction: 1 - (1 - a')^n of the n samples inside"""
    shape, spacing = (20, 16, 16), (1.0, 1.0, 1.0)
    field = np.full(shape, 1000, np.uint16)
    p = dict(PRESETS["Standard"])
    cam = V.camera_for_view("top", shape, spacing, (16, 16))
    s = V.render_setup(p, (-1024, 3071), cam, color_lists=CLUTS)
    s["shade"] = False
    img = R.render(field, spacing, s)
    n = int(np.floor((shape[0] - 1) / s["dt"])) + 1
    ap = s["rgba"][1000, 3]
    expect = 1 - (1 - ap) ** n
    inside = img[4:-4, 4:-4, 3]
    assert np.allclose(inside, expect, rtol=0, atol=1e-12)


def _voxel_top_camera(shape, pitch):
    """the top view with pixel pitch = the x / y spacing and one pixel of margin around odd x / y axes: every pixel
    centre sits on a voxel column, the rim ones inside the x / y faces, the ring around them just outside the box"""
    size = (shape[2] + 2, shape[1] + 2)
    return dict(V.camera_for_view("top", shape, (pitch, pitch, 1.0), size), parallel_scale=size[1] * pitch / 2.0)


def _ring(img):
    r = np.ones(img.shape[:2], bool)
    r[1:-1, 1:-1] = False
    return r


def _value_with_opacity(target):
    """the field value whose baked a' (Standard at scale (-1024, 3071)) is nearest `target`"""
    s = V.render_setup(PRESETS["Standard"], (-1024, 3071), _voxel_top_camera((3, 9, 11), 0.75), color_lists=CLUTS)
    return int(np.argmin(np.abs(s["rgba"][:4096, 3] - target)))


def _uniform_top(value, nz, **kw):
    shape, spacing = (nz, 9, 11), (0.75, 0.75, 1.0)
    s = V.render_setup(PRESETS["Standard"], (-1024, 3071), _voxel_top_camera(shape, 0.75), color_lists=CLUTS, **kw)
    s["shade"] = False
    w, h = s["viewport"]
    py, px = np.mgrid[0:h, 0:w]
    p = s["origin"] + px[..., None] * s["du"] + py[..., None] * s["dv"]
    assert np.array_equal(np.unique(p[..., 0] / 0.75), np.arange(-1.0, 12.0))  # A_x: -1, 0 .. 10, 11
    assert np.array_equal(np.unique(-p[..., 1] / 0.75), np.arange(-1.0, 10.0))  # A_y: -1, 0 .. 8, 9
    return R.render(np.full(shape, value, np.uint16), spacing, s), s


@pytest.mark.parametrize("nz", [20, 2, 1])
def test_oracle_uniform_box_every_ray_closed_form(nz):
    """every ray that hits the uniform box, the rim in the faces included, composites its n = floor((nz - 1) / dt) + 1
    samples to 1 - (1 - a')^n (one sample for a one-voxel axis); the ring outside is background"""
    v = _value_with_opacity(0.02)
    img, s = _uniform_top(v, nz)
    n = int(np.floor((nz - 1) / s["dt"])) + 1
    assert n == {20: 48, 2: 3, 1: 1}[nz]
    ap, c, bg = s["rgba"][v, 3], s["rgba"][v, :3], np.array(s["background"])
    expect = 1 - (1 - ap) ** n
    assert 0.01 < ap < 0.03 and expect < R.OPAQUE
    inside = img[1:-1, 1:-1]
    assert np.allclose(inside[..., 3], expect, rtol=0, atol=1e-12)
    assert np.allclose(inside[..., :3], c * expect + (1 - expect) * bg, rtol=0, atol=1e-12)
    ring = img[_ring(img)]
    assert np.all(ring[:, 3] == 0) and np.all(ring[:, :3] == bg)


def test_oracle_clip_plane_sample_count():
    """the uniform box from the top, cut by the plane z = 2.9 (kept: z <= 2.9): the samples start on the plane, so a ray
    takes floor(2.9 / dt) + 1 = 8 of them"""
    v = _value_with_opacity(0.02)
    img, s = _uniform_top(v, 20, clip_plane=((0.0, 0.0, -1.0), (0.0, 0.0, 2.9)))
    ap = s["rgba"][v, 3]
    assert ap > 0.01 and np.allclose(img[1:-1, 1:-1, 3], 1 - (1 - ap) ** 8, rtol=0, atol=1e-12)
    assert np.all(img[_ring(img)][:, 3] == 0)


def test_oracle_early_termination_closed_form():
    """a uniform box with a' near 0.5: a ray stops at the first sample m with 1 - (1 - a')^m >= 1 - 2^-12, well before
    its 48 samples, so the pixel is 1 - (1 - a')^m and not 1 - (1 - a')^48"""
    v = _value_with_opacity(0.5)
    img, s = _uniform_top(v, 20)
    ap, c, bg = s["rgba"][v, 3], s["rgba"][v, :3], np.array(s["background"])
    m = next(k for k in range(1, 49) if 1 - (1 - ap) ** k >= R.OPAQUE)
    expect = 1 - (1 - ap) ** m
    assert 0.3 < ap < 0.7 and m < 48 and expect - (1 - (1 - ap) ** 48) < -1e-5
    assert np.allclose(img[1:-1, 1:-1, 3], expect, rtol=0, atol=1e-12)
    assert np.allclose(img[1:-1, 1:-1, :3], c * expect + (1 - expect) * bg, rtol=0, atol=1e-12)


def test_synth_volume_shell():
    def faces(v):
        return (v[0], v[-1], v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1])

    shell3, shell0 = R.synth_volume((20, 24, 28), seed=2), R.synth_volume((20, 24, 28), seed=2, shell=0)
    assert all(np.all(f == -1024) for f in faces(shell3))
    assert all(np.count_nonzero(f != -1024) > f.size // 2 for f in faces(shell0))  # shell 0 keeps the faces
    inner0, inner3 = shell0[3:-3, 3:-3, 3:-3].copy(), shell3[3:-3, 3:-3, 3:-3]
    inner0[0, 0, 0] = -1024  # shell 3's corner marker
    assert np.array_equal(inner0, inner3)


@pytest.mark.parametrize("shape", [(22, 30, 36), (1, 20, 23), (16, 1, 9), (12, 33, 1)], ids=str)
def test_cropped_ct_has_material_on_its_faces(shape):
    ct = R.cropped_ct(shape, seed=1)
    assert ct.min() == -1024 and ct.max() == 3071
    for z_face in (ct[0], ct[-1]):  # the body runs through the first and last slice
        assert np.count_nonzero(z_face > -500) > z_face.size // 3
    if shape[1] >= 2:  # the table: the whole y = ny - 1 face, and into both x faces
        assert np.all(ct[:, -1] >= 1000)
        assert np.count_nonzero(ct[:, :, 0] >= 1000) >= shape[0] and np.count_nonzero(ct[:, :, -1] >= 1000) >= shape[0]


def test_oracle_mip_closed_form():
    """an axis-aligned MIP with dt = spacing gives the maximum along the axis"""
    rng = np.random.default_rng(3)
    shape, spacing = (12, 9, 10), (1.0, 1.0, 1.0)
    field = rng.integers(0, 4000, shape).astype(np.uint16)
    p = PRESETS["MIP"]
    cam = V.camera_for_view("top", shape, spacing, (10, 9))
    s = V.render_setup(p, (-1024, 3071), cam, dt=1.0)
    # pixel (i, j) of a top view at this size sits on voxel column (y = j, x = i) when the scale is one voxel per pixel
    cam = dict(cam, parallel_scale=4.5)
    s = V.render_setup(p, (-1024, 3071), cam, dt=1.0)
    img = R.render(field, spacing, s)
    mx = field.max(0).astype(np.int64)
    e = s["rgba"][mx]
    a = s["alpha"][mx]
    bg = np.array(s["background"])
    expect = a[..., None] * e[..., :3] + (1 - a[..., None]) * bg
    assert np.allclose(img[..., :3], expect, atol=1e-12)


def test_prepare_restatement_truncates():
    """the 5x5 pass of a constant region gives v - 1 for some v: the float64 sum of k / 60.0 weights falls short"""
    w = V.convolution_kernels(PRESETS["Bone + Skin"])
    vals = np.arange(0, 65536, 1, dtype=np.int64)
    img = np.repeat(vals[:, None, None], 5, 1).repeat(5, 2)  # (65536, 5, 5): one constant slice per value
    out = R.prepare((img - 32768).astype(np.int16), 32768, w)[:, 2, 2]
    low = np.count_nonzero(out.astype(np.int64) == vals - 1)
    assert low == 30284 and np.count_nonzero(out == vals) == 65536 - 30284


def test_png_roundtrip(tmp_path):
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (7, 9, 4)).astype(np.uint8)
    V.write_png(str(tmp_path / "a.png"), img)
    assert np.array_equal(V.read_png(str(tmp_path / "a.png")), img)
    assert np.array_equal(V.to_rgba8(np.array([0.0, 0.5, 1.0, 1.2, -0.1, 0.998])), [0, 128, 255, 255, 0, 254])
