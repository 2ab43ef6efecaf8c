"""CPU: the host side of the mask 3-D preview (invesalius3_amd/volume_mask.py) against the calls the reference itself
makes (tests/golden/ref_maskpreview.npz, recorded by make_golden_ref_maskpreview.py), its geometry, the baked table, and
the float64 oracle of tests/_maskren_ref.py on hand-built rays with closed-form hits."""
import json
import os

import numpy as np
import pytest

import _maskren_ref as MR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_maskpreview.npz")
RUNS = json.loads(str(np.load(GOLDEN)["runs_json"]))
VIEWS = ["front", "back", "left", "right", "top", "bottom", "iso"]


def _nodes(calls, kind, method):
    """the node list VTK holds after `calls`: the Add* calls behind the last RemoveAllPoints, replayed"""
    from invesalius3_amd import volume as V
    n = V.Nodes()
    for c in calls:
        if c[0] != kind:
            continue
        if c[1] == "RemoveAllPoints":
            n = V.Nodes()
        elif c[1] == method:
            n.add(*c[2])
    return n.array()


def _args(calls, kind, method):
    return [c[2] for c in calls if c[0] == kind and c[1] == method]


def test_fixture_covers_both_renderings_and_three_colours():
    assert sorted({r["rendering"] for r in RUNS}) == [0, 1]
    assert len({tuple(r["colour"]) for r in RUNS}) == 3 and len(RUNS) == 6


@pytest.mark.parametrize("run", RUNS, ids=lambda r: "rendering%d-%s" % (r["rendering"], r["colour"]))
def test_preview_setup_equals_the_recorded_calls(run):
    from invesalius3_amd import volume_mask as VM
    calls = run["create_volume"]
    mode = "iso" if run["rendering"] else "composite"
    ps = VM.preview_setup(run["colour"], mode)
    assert np.array_equal(ps["colour_nodes"].array(), _nodes(calls, "ctf", "AddRGBPoint"))
    assert np.array_equal(ps["opacity_nodes"].array(), _nodes(calls, "pwf", "AddPoint"))
    # the property: what is set equals the setup, what is not set is VTK's default
    assert bool(_args(calls, "prop", "ShadeOn")) == ps["shade"]
    assert bool(_args(calls, "prop", "SetInterpolationTypeToLinear")) == (ps["interpolation"] == "linear")
    assert _args(calls, "prop", "SetSpecular") == [[ps["specular"]]]
    assert _args(calls, "prop", "SetSpecularPower") == [[ps["specular_power"]]]
    assert not _args(calls, "prop", "SetAmbient") and not _args(calls, "prop", "SetDiffuse")
    assert (ps["ambient"], ps["diffuse"]) == (0.1, 0.7)
    # the mapper and the mode
    mapper = {"vtkFixedPointVolumeRayCastMapper": "mapper_fixedpoint", "vtkGPUVolumeRayCastMapper": "mapper_gpu"}[ps["mapper"]]
    assert {c[0] for c in calls if c[0].startswith("mapper")} == {mapper}
    assert bool(_args(calls, mapper, "UseJitteringOn")) == ps["jitter"]
    assert bool(_args(calls, mapper, "IntermixIntersectingGeometryOn")) == ps["intermix_geometry"]
    assert bool(_args(calls, mapper, "SetBlendModeToIsoSurface")) == (ps["blend"] == "iso_surface")

    def one(kind, method):
        a = _args(calls, kind, method)
        return a[0][-1] if a else None

    assert one(mapper, "SetSampleDistance") == ps["sample_distance"]
    assert one(mapper, "SetImageSampleDistance") == ps["image_sample_distance"]
    assert one("prop", "SetScalarOpacityUnitDistance") == ps["opacity_unit_distance"]
    assert one("isovalues", "SetValue") == ps["iso_value"]
    if mode == "iso":
        assert _args(calls, "isovalues", "SetValue") == [[0, VM.ISO_VALUE]]
    # the flip of the geometry: axis 1 about the origin
    assert _args(calls, "flip", "SetFilteredAxis") == [[1]] and _args(calls, "flip", "FlipAboutOriginOn") == [[]]
    # set_colour rebuilds the colour nodes only
    for sc in run["set_colour"]:
        assert {c[0] for c in sc["calls"]} == {"ctf"}
        assert np.array_equal(VM.preview_setup(sc["colour"], mode)["colour_nodes"].array(),
                              _nodes(sc["calls"], "ctf", "AddRGBPoint"))


def test_unknown_mode_is_an_error():
    from invesalius3_amd import volume_mask as VM
    with pytest.raises(ValueError):
        VM.preview_setup((1, 0, 0), "mip")


def test_interior_coincides_with_the_image_and_the_box_spans_the_matrix():
    from invesalius3_amd import volume as V
    from invesalius3_amd import volume_mask as VM
    shape, spacing = (5, 7, 9), (0.7, 0.9, 1.3)
    mshape = tuple(s + 1 for s in shape)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    img_world = np.stack([x * spacing[0], -y * spacing[1], z * spacing[2]], -1)  # volume.volume_bounds' rule
    assert np.array_equal(VM.voxel_world((z + 1, y + 1, x + 1), spacing), img_world)
    b = V.volume_bounds(shape, spacing)
    assert np.allclose([img_world[..., 0].min(), img_world[..., 0].max(), img_world[..., 1].min(),
                        img_world[..., 1].max(), img_world[..., 2].min(), img_world[..., 2].max()], b, atol=1e-12, rtol=0)
    zz, yy, xx = np.meshgrid(*[np.arange(n) for n in mshape], indexing="ij")
    w = VM.voxel_world((zz, yy, xx), spacing)
    box = VM.preview_bounds(mshape, spacing)
    assert np.allclose([w[..., 0].min(), w[..., 0].max(), w[..., 1].min(), w[..., 1].max(), w[..., 2].min(),
                        w[..., 2].max()], box, atol=1e-12, rtol=0)
    # the near faces lie one spacing outside the image's box, the far faces on it
    assert np.allclose(box, (-spacing[0], b[1], b[2], spacing[1], -spacing[2], b[5]), atol=1e-12, rtol=0)


def test_render_setup_moves_the_origin_so_that_the_oracle_sees_the_padded_index():
    """index = world / spacing + 1 on every axis: the rays' box of the oracle is the box of preview_bounds"""
    from invesalius3_amd import volume as V
    from invesalius3_amd import volume_mask as VM
    shape, spacing = (6, 5, 8), (0.8, 1.1, 0.6)
    cam = V.camera_for_view("iso", shape, spacing, (9, 7))
    st = VM.render_setup((0, 1, 0), "iso", cam, spacing)
    origin, du, dv = V.pixel_rays(cam)
    assert np.array_equal(st["origin"], origin + np.array([spacing[0], -spacing[1], spacing[2]]))
    assert st["dt"] == 0.5 * min(spacing)
    assert VM.render_setup((0, 1, 0), "composite", cam, spacing)["dt"] == 2.0 / 5
    assert VM.render_setup((0, 1, 0), "iso", cam, spacing, sample_distance=0.25)["dt"] == 0.25


@pytest.mark.parametrize("colour", [(0.0, 1.0, 0.0), (0.33, 0.25, 0.9), (1.0, 0.5, 0.125)])
def test_table_is_the_nodes_evaluated_per_byte(colour):
    from invesalius3_amd import volume as V
    from invesalius3_amd import volume_mask as VM
    cam = V.camera_for_view("front", (4, 4, 4), (1, 1, 1), (8, 8))
    st = VM.render_setup(colour, "composite", cam, (1, 1, 1))
    q = np.arange(257, dtype=np.float64)
    ps = st["preview"]
    assert st["rgba"].shape == (257, 4) and st["prefix"].shape == (258,)
    assert np.array_equal(st["rgba"][:, :3], np.clip(ps["colour_nodes"].evaluate(q), 0, 1))
    a = np.clip(ps["opacity_nodes"].evaluate(q)[:, 0], 0, 1)
    assert np.array_equal(st["alpha"], a)
    assert a[0] == 0 and a[127] == 1 and a[256] == 1 and np.all(np.diff(a[:128]) > 0)
    assert np.array_equal(st["rgba"][:, 3], 1.0 - np.power(1.0 - a, 0.4 / 2.0))
    assert st["prefix"][1] == 0 and st["prefix"][2] == 1  # only byte 0 is transparent
    iso = VM.render_setup(colour, "iso", cam, (1, 1, 1))
    assert np.array_equal(iso["rgba"][127, :3], ps["colour_nodes"].evaluate([127.0])[0])
    assert np.allclose(iso["rgba"][127, :3], np.array(colour) * 127 / 254, atol=1e-15, rtol=0)


# -- the oracle on hand-built rays ------------------------------------------------------------------------------------
def _one_ray(matrix, spacing, world_start, direction, dt=None, mode="iso"):
    """the oracle on one ray that starts at `world_start` (a 1 x 1 viewport whose only pixel centre is the focal point)"""
    from invesalius3_amd import volume_mask as VM
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    up = np.array([0.0, 0.0, 1.0]) if abs(d[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(d, up)
    right /= np.linalg.norm(right)
    cam = {"focal": np.asarray(world_start, np.float64), "dir": d, "right": right, "up": np.cross(right, d),
           "parallel_scale": 1.0, "viewport": (1, 1)}
    st = VM.render_setup((0.2, 0.9, 0.4), mode, cam, spacing, background=(0.1, 0.2, 0.3), sample_distance=dt)
    res = MR.render(matrix, spacing, st)
    return {k: v.reshape(v.shape[2:] if k == "image" else ()) for k, v in res.items()}, st


def _world(z, y, x, spacing):
    from invesalius3_amd import volume_mask as VM
    return VM.voxel_world((z, y, x), spacing)


SP = (0.8, 1.1, 1.3)


def test_ray_through_a_single_voxel():
    m = np.zeros((9, 9, 12), np.uint8)
    m[4, 5, 6] = 255
    start = _world(4, 5, -5, SP)  # five voxels in front of the box, on the row through the voxel
    res, st = _one_ray(m, SP, start, (1, 0, 0), dt=0.4)  # 0.4 / 0.8: two samples per voxel, on and between the centres
    # along the row f is linear from 0 at x = 5 to 255 at x = 6: it crosses 127 at x = 5 + 127 / 255
    assert res["depth"] == pytest.approx((5 + 5 + 127 / 255) * SP[0], abs=1e-12)
    assert res["image"][3] == 1.0
    # the gradient there points along x only: n . l = 1, colour nodes at 127, shaded
    c = st["rgba"][127, :3]
    assert np.allclose(res["image"][:3], np.clip(c * (0.1 + 0.7) + 0.75, 0, 1), atol=1e-12, rtol=0)
    # a row beside the voxel's support never reaches 127: the background with alpha 0
    miss, _ = _one_ray(m, SP, _world(4, 7, -5, SP), (1, 0, 0), dt=0.4)
    assert np.isinf(miss["depth"]) and np.array_equal(miss["image"], [0.1, 0.2, 0.3, 0.0])


def test_ray_into_a_slab_from_both_sides():
    m = np.zeros((8, 8, 14), np.uint8)
    m[:, :, 5:9] = 255
    res, _ = _one_ray(m, SP, _world(3, 4, -2, SP), (1, 0, 0), dt=0.4)
    assert res["depth"] == pytest.approx((2 + 4 + 127 / 255) * SP[0], abs=1e-12)
    back, _ = _one_ray(m, SP, _world(3, 4, 16, SP), (-1, 0, 0), dt=0.4)  # f = 255 (9 - x) between 8 and 9
    assert back["depth"] == pytest.approx((16 - (9 - 127 / 255)) * SP[0], abs=1e-12)
    # along y (world -y) and z likewise
    m2 = np.zeros((12, 10, 6), np.uint8)
    m2[:, 4:7, :] = 255
    ry, _ = _one_ray(m2, SP, _world(5, -3, 2, SP), (0, -1, 0), dt=0.55)
    assert ry["depth"] == pytest.approx((3 + 3 + 127 / 255) * SP[1], abs=1e-12)


def test_ray_that_starts_inside_material_at_a_far_face_hits_where_it_leaves():
    m = np.zeros((8, 8, 12), np.uint8)
    m[:, :, 6:] = 255  # up to the far x face, which no flag plane closes
    res, _ = _one_ray(m, SP, _world(3, 4, 15, SP), (-1, 0, 0), dt=0.4)
    # the first sample, on the face, is inside (255); f = 255 (x - 5) between 5 and 6 falls through 127 at 5 + 127 / 255
    assert res["depth"] == pytest.approx((15 - (5 + 127 / 255)) * SP[0], abs=1e-12)
    assert res["image"][3] == 1.0


@pytest.mark.parametrize("flag", [0, 1, 2])
def test_ray_through_the_flag_plane_in_front_of_material(flag):
    mask = np.full((6, 6, 6), 255, np.uint8)
    m = MR.padded(mask, flag)
    res, _ = _one_ray(m, SP, _world(3, 3, -4, SP), (1, 0, 0), dt=0.4)
    # the box starts on the flag plane (x = 0, value `flag`); f rises linearly to 255 at x = 1
    assert res["depth"] == pytest.approx((4 + (127 - flag) / (255 - flag)) * SP[0], abs=1e-12)


def test_sample_exactly_at_127_is_the_hit():
    m = np.zeros((8, 8, 12), np.uint8)
    m[:, :, 4] = 127
    m[:, :, 5:] = 254
    res, _ = _one_ray(m, SP, _world(3, 4, -3, SP), (1, 0, 0), dt=0.4)
    # samples at x = 0, 0.5, 1, ...: f(3.5) = 63.5, f(4) == 127 exactly -- the hit is that sample, no interpolation
    assert res["depth"] == pytest.approx((3 + 4) * SP[0], abs=1e-12)
    assert res["margin"] == 0.0
    # a first sample at 127 is no hit by itself (k >= 1): the ray goes on to a crossing
    m2 = np.zeros((8, 8, 12), np.uint8)
    m2[:, :, 0] = 127
    m2[:, :, 6:] = 255
    res2, _ = _one_ray(m2, SP, _world(3, 4, -3, SP), (1, 0, 0), dt=0.4)
    assert res2["depth"] == pytest.approx((3 + 5 + 127 / 255) * SP[0], abs=1e-12)


def test_composite_ray_is_the_volume_oracle_on_bytes():
    import _volren_ref as R
    m = MR.padded(MR.levels_mask((6, 7, 8)), 1)
    res, st = _one_ray(m, SP, _world(3, 3, -4, SP), (1, 0.2, 0.1), mode="composite")
    assert np.array_equal(res["image"], R.render(m, SP, st).reshape(4))
    assert 0 < res["image"][3] <= 1


# -- the inputs of the GPU comparison keep float32 and float64 apart only on the rays it leaves out ---------------------
@pytest.mark.parametrize("case", MR.gpu_iso_inputs(), ids=lambda c: c[0])
def test_float32_stepping_stays_inside_the_exclusion_cap(case):
    """The iso oracle in emulated float32 against itself in float64 on every input the GPU module compares in the iso mode:
    outside the rays whose margin is below eps the two agree on hit or miss, the colour stays inside 1e-3 and the depth
    inside the position bound, and the excluded share is at most 1 % of the rays that hit the box."""
    from invesalius3_amd import volume as V
    from invesalius3_amd import volume_mask as VM
    tag, m, spacing, view, size, kw = case
    shape = tuple(s - 1 for s in m.shape)
    cam = V.camera_for_view(view, shape, spacing, size)
    st = VM.render_setup((0.0, 1.0, 0.0), "iso", cam, spacing, **kw)
    r64, r32 = MR.render(m, spacing, st), MR.render(m, spacing, st, f32=True)
    delta, count = MR.position_bound(m.shape, spacing, st)
    eps = delta * MR.max_slope(m)
    keep = MR.compare_mask(r64, eps)
    excluded = np.count_nonzero(r64["in_box"] & ~keep) / max(np.count_nonzero(r64["in_box"]), 1)
    assert excluded <= 0.01, (excluded, eps)
    assert np.array_equal(np.isinf(r64["depth"][keep]), np.isinf(r32["depth"][keep]))
    hit = keep & np.isfinite(r64["depth"])
    err = np.abs(r64["depth"][hit] - r32["depth"][hit])
    assert err.max(initial=0.0) <= delta * max(spacing)
    assert np.abs(r64["image"][keep] - r32["image"][keep]).max(initial=0.0) <= 1e-3


@pytest.mark.parametrize("case", MR.gpu_iso_inputs(), ids=lambda c: c[0])
def test_composite_inputs_have_no_degenerate_gradient(case):
    """the composite comparison's precondition (tests/_maskren_ref.noise_gradients), checked before a GPU run"""
    from invesalius3_amd import volume as V
    from invesalius3_amd import volume_mask as VM
    tag, m, spacing, view, size, kw = case
    kw = {k: v for k, v in kw.items() if k != "sample_distance"}
    cam = V.camera_for_view(view, tuple(s - 1 for s in m.shape), spacing, size)
    assert MR.noise_gradients(m, spacing, VM.render_setup((0.0, 1.0, 0.0), "composite", cam, spacing, **kw)) == 0
