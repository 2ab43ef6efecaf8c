"""The surface view on the GPU (csrc/k_surfview.hip) through libivx.so, against the numpy restatement of rules
R1 - R5 (tests/_surface_view_ref.py) on every case of tests/_surface_view_cases.py.

Every comparison is np.array_equal -- keys, ids, depth BITS, float32 RGBA bits and RGBA8, with nothing excluded: the
arithmetic is float64 + - * / sqrt in one stated order on both sides, the nearest fragment is a 64-bit unsigned minimum whose
result does not depend on arrival order, and the composition is sorted, so there is nothing to tolerate."""
import ctypes
import functools

import numpy as np
import pytest

import _surface_view_cases as C
import _surface_view_ref as R

pytestmark = pytest.mark.gpu

BACKGROUND = (0.125, 0.25, 0.5)
SCENES = {s["name"]: s for s in C.scenes()}
MODES = {"flat": R.FLAT, "gouraud": R.GOURAUD, "phong": R.PHONG}


@functools.lru_cache(maxsize=None)
def ref_keys(name):
    s = SCENES[name]
    return tuple(R.raster_keys(m["verts"], m["faces"], s["cam"]) for m in s["layers"])


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """the restatement's picture of a case: computed once, shared, never modified"""
    s = SCENES[name]
    out = R.render(s["layers"], s["cam"], mode, BACKGROUND, keys=list(ref_keys(name)))
    for k in ("rgba", "rgba8", "ids", "depth"):
        out[k].setflags(write=False)
    return out


@pytest.fixture(scope="module")
def SV(ivxlib):
    from invesalius3_amd import surface_view
    return surface_view


def actors_of(SV, layers):
    return [SV.SurfaceActor(m["verts"], m["faces"], m["normals"], m["colour"], m["transparency"]) for m in layers]


def assert_picture(got, want, what):
    for k in ("ids", "depth", "rgba"):
        a, b = np.ascontiguousarray(got[k]), want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        bad = np.nonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(a.shape[0], a.shape[1], -1).any(axis=-1))
        assert not len(bad[0]), "%s: %d pixels of %s differ, first at (row %d, column %d): %r vs %r" % (
            what, len(bad[0]), k, bad[0][0], bad[1][0], a[bad[0][0], bad[1][0]], b[bad[0][0], bad[1][0]])


# ---- 1: every case, host form and device-resident form -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_case_equals_the_restatement(SV, name):
    s = SCENES[name]
    size = s["cam"]["viewport"]
    modes = MODES.values() if (name.startswith("icosphere") or "inside" in name or name in ("degenerate", "eight surfaces")) else (R.GOURAUD,)
    with SV.Scene(actors_of(SV, s["layers"])) as scene:
        for mode in modes:
            want = reference(name, mode)
            host = SV.render_surfaces(actors_of(SV, s["layers"]), s["cam"], size, interpolation=mode, background=BACKGROUND, depth=True, ids=True)
            assert_picture(host, want, "%s, mode %d, host form" % (name, mode))
            dev = scene.render(s["cam"], size, interpolation=mode, background=BACKGROUND, depth=True, ids=True)
            assert_picture(dev, want, "%s, mode %d, resident form" % (name, mode))
            u8 = scene.render(s["cam"], size, interpolation=mode, background=BACKGROUND, rgba8=True)
            assert u8.dtype == np.uint8 and np.array_equal(u8, want["rgba8"])
            assert np.array_equal(SV.render_surfaces(actors_of(SV, s["layers"]), s["cam"], size, interpolation=mode, background=BACKGROUND,
                                                     rgba8=True), want["rgba8"])
        for k, keys in enumerate(ref_keys(name)):
            assert np.array_equal(scene.download_keys(k), keys), "%s: keys of surface %d" % (name, k)
        assert scene.raster_runs == len(s["layers"])  # one raster per surface, whatever the number of renders


def test_nine_surfaces_is_einval(SV):
    layers = C.eight_layers(9)
    with pytest.raises(TypeError):
        SV.render_surfaces(actors_of(SV, layers), C.hand_cam(), (16, 16))
    from invesalius3_amd import _lib as L
    cc = SV._c_camera(C.hand_cam())
    arr = (SV.SurfaceLayer * 9)()
    out = np.zeros((16, 16, 4), np.float32)
    bg = (ctypes.c_float * 3)(0, 0, 0)
    assert L.lib().ivx_surface_render(arr, 9, ctypes.byref(cc), 1, bg, 0, L.ptr(out), None, None) == L.IVX_EINVAL
    assert L.lib().ivx_dev_surface_resolve(arr, 9, ctypes.byref(cc), 1, bg, 0, L.ptr(out), None, None, None) == L.IVX_EINVAL
    # eight visible ones of nine are a scene
    actors = actors_of(SV, layers)
    actors[8].visible = False
    cam = SCENES["eight surfaces"]["cam"]
    got = SV.render_surfaces(actors, cam, cam["viewport"], background=BACKGROUND, depth=True, ids=True)
    assert_picture(got, reference("eight surfaces", R.GOURAUD), "eight of nine")


# ---- 2: determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere iso", "eight surfaces", "cube 256"])
def test_two_renders_give_the_same_bytes(SV, name):
    s = SCENES[name]
    a = SV.render_surfaces(actors_of(SV, s["layers"]), s["cam"], s["cam"]["viewport"], depth=True, ids=True)
    b = SV.render_surfaces(actors_of(SV, s["layers"]), s["cam"], s["cam"]["viewport"], depth=True, ids=True)
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("rgba", "depth", "ids"))


@pytest.mark.parametrize("name", [n for n, s in SCENES.items() if not s["ties"] and s["layers"] and sum(len(m["faces"]) for m in s["layers"]) > 1])
def test_shuffled_launch_order_gives_the_same_picture(SV, name):
    s = SCENES[name]
    rng = np.random.default_rng(11)
    perms = [rng.permutation(len(m["faces"])) for m in s["layers"]]
    shuffled = [dict(m, faces=np.ascontiguousarray(m["faces"][p])) for m, p in zip(s["layers"], perms)]
    got = SV.render_surfaces(actors_of(SV, shuffled), s["cam"], s["cam"]["viewport"], background=BACKGROUND, depth=True, ids=True)
    ids = got["ids"].copy()
    for k, p in enumerate(perms):
        sel = ids[..., 0] == k
        ids[..., 1][sel] = p[ids[..., 1][sel]]  # back through the permutation
    assert_picture({"ids": ids, "depth": got["depth"], "rgba": got["rgba"]}, reference(name, R.GOURAUD), name + ", shuffled")


# ---- 3: the stages apart ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box 64 x 1", "box 65 x 1", "cube 256", "icosphere iso"])
def test_stages_run_apart_equal_one_call(SV, name):
    from invesalius3_amd import _lib as L
    from invesalius3_amd import polydata_utils as pu
    from invesalius3_amd.device import DeviceBuffer
    s = SCENES[name]
    m = s["layers"][0]
    W, H = s["cam"]["viewport"]
    cc = SV._c_camera(s["cam"])
    mesh = pu.DeviceMesh.upload(m["verts"], m["faces"])
    keys = DeviceBuffer(W * H * 8)
    try:
        seen = []
        for stages in (SV.RASTER_CLEAR, SV.RASTER_SMALL, SV.RASTER_BIG):
            L.check(L.lib().ivx_dev_surface_raster(mesh.verts.ptr, ctypes.c_int64(mesh.nverts), mesh.faces.ptr, ctypes.c_int64(mesh.ntris),
                                                   ctypes.byref(cc), stages, keys.ptr, None))
            L.synchronize()
            seen.append(keys.download((H, W), np.uint64))
        assert (seen[0] == R.EMPTY).all() and np.array_equal(seen[2], ref_keys(name)[0])
        small_only = name in ("box 64 x 1", "icosphere iso")  # 64 pixels: the lane's; 65: the workgroup's
        assert np.array_equal(seen[1], seen[2]) == small_only
        if name in ("box 65 x 1", "cube 256"):
            assert (seen[1] == R.EMPTY).all()
    finally:
        keys.close()
        mesh.close()


# ---- 4: a Scene keeps its keys -------------------------------------------------------------------------------------------------------
def test_colour_and_transparency_changes_run_the_resolve_only(SV):
    s = SCENES["opaque inside translucent iso"]
    cam, size = s["cam"], s["cam"]["viewport"]
    actors = actors_of(SV, s["layers"])
    with SV.Scene(actors) as scene:
        scene.render(cam, size, background=BACKGROUND)
        assert scene.raster_runs == 2 and scene.last_stages == [SV.RASTER_ALL, SV.RASTER_ALL]
        actors[0].colour, actors[0].transparency, actors[1].colour = (0.25, 0.5, 1.0), 0.3, (1.0, 1.0, 0.33)
        got = scene.render(cam, size, background=BACKGROUND, depth=True, ids=True)
        assert scene.raster_runs == 2 and scene.last_stages == [0, 0]  # no stage of the rasteriser ran
        layers = [dict(s["layers"][0], colour=(0.25, 0.5, 1.0), transparency=0.3, opacity=np.float32(0.7)), dict(s["layers"][1], colour=(1.0, 1.0, 0.33))]
        assert_picture(got, R.render(layers, cam, R.GOURAUD, BACKGROUND, keys=list(ref_keys(s["name"]))), "after the change")
        scene.render(cam, size, interpolation="phong", background=(0, 0, 0), rgba8=True)
        assert scene.raster_runs == 2 and scene.last_stages == [0, 0]
        # hiding a surface rasterises nothing either; another camera rasterises what is visible
        actors[0].visible = False
        alone = scene.render(cam, size, background=BACKGROUND, depth=True, ids=True)
        assert scene.raster_runs == 2 and scene.last_stages == [0]
        assert_picture(alone, R.render([layers[1]], cam, R.GOURAUD, BACKGROUND), "one hidden")
        other = SCENES["opaque inside translucent top"]["cam"]
        scene.render(other, size)
        assert scene.raster_runs == 3 and scene.last_stages == [SV.RASTER_ALL]


# ---- 5: picking -----------------------------------------------------------------------------------------------------------------------
def test_pick_on_the_hand_built_cases(SV):
    from invesalius3_amd import resident
    verts, faces = C.hand_triangle(t=(3.0, 1.0, 7.0))
    cam = C.hand_cam()
    with SV.Scene([SV.SurfaceActor(verts, faces)]) as scene:
        scene.render(cam, (16, 16))
        before = resident.transfer_stats()
        hit = scene.pick(2, 2)  # the corner a itself
        after = resident.transfer_stats()
        assert after["d2h_bytes"] - before["d2h_bytes"] == 60 and after["h2d_bytes"] == before["h2d_bytes"]
        assert (hit["surface"], hit["triangle"], hit["point_id"]) == (0, 0, 0)
        assert np.array_equal(hit["position"], np.float64(verts[0]))
        hit = scene.pick(2, 6)
        assert hit["point_id"] == 1 and np.array_equal(hit["position"], np.float64(verts[1]))
        hit = scene.pick(5, 3)  # centre (5.5, 3.5): t = 3 + 3 - 0.5, nearest to corner c
        assert hit["point_id"] == 2 and np.array_equal(hit["position"], np.array(C.at_screen(5.5, 3.5, 5.5)))
        assert scene.pick(10, 10) is None
        with pytest.raises(IndexError):
            scene.pick(16, 0)
    s = SCENES["translucent inside opaque iso"]
    with SV.Scene(actors_of(SV, s["layers"])) as scene:
        scene.render(s["cam"], s["cam"]["viewport"])
        want = reference(s["name"], R.GOURAUD)
        for col, row in ((32, 32), (20, 40), (0, 0), (45, 18)):
            a, b = scene.pick(col, row), R.pick(want, s["cam"], s["layers"], col, row)
            assert (a is None) == (b is None)
            if a is not None:
                assert (a["surface"], a["triangle"], a["point_id"]) == (b["surface"], b["triangle"], b["point_id"])
                assert np.allclose(a["position"], b["position"], rtol=0, atol=1e-12)


# ---- 6: what crosses the link ---------------------------------------------------------------------------------------------------------
def test_device_resident_render_moves_only_the_picture(SV):
    from invesalius3_amd import polydata_utils as pu
    from invesalius3_amd import resident
    from invesalius3_amd.device import DeviceBuffer
    s = SCENES["icosphere iso"]
    m = s["layers"][0]
    W, H = s["cam"]["viewport"]
    mesh = pu.DeviceMesh.upload(m["verts"], m["faces"])
    normals = DeviceBuffer(m["normals"].nbytes)
    normals.upload(m["normals"])
    try:
        with SV.Scene([SV.SurfaceActor(mesh, normals=normals, colour=m["colour"])]) as scene:
            before = resident.transfer_stats()
            got = scene.render(s["cam"], (W, H), background=BACKGROUND, rgba8=True)
            after = resident.transfer_stats()
            assert after["h2d_bytes"] == before["h2d_bytes"]                   # camera and layers travel as kernel arguments
            assert after["d2h_bytes"] - before["d2h_bytes"] == W * H * 4       # the RGBA8 picture, nothing else
            assert np.array_equal(got, reference(s["name"], R.GOURAUD)["rgba8"])
            before = after
            bufs = scene.render(s["cam"], (W, H), background=BACKGROUND, download=False)
            assert resident.transfer_stats() == before and isinstance(bufs["rgba"], DeviceBuffer)
        # the one-actor shorthand, with the camera from the mesh's own bounds
        got = mesh.render(normals=normals, colour=m["colour"], camera="iso", size=(W, H), background=BACKGROUND, depth=True, ids=True)
        assert_picture(got, reference(s["name"], R.GOURAUD), "DeviceMesh.render")
    finally:
        normals.close()
        mesh.close()


def test_camera_of_an_image_and_of_the_scene(SV):
    from invesalius3_amd import volume as V
    s = SCENES["icosphere front"]
    m = s["layers"][0]
    actors = actors_of(SV, s["layers"])
    assert np.array_equal(SV.render_surfaces(actors, "front", (96, 96), background=BACKGROUND), reference(s["name"], R.GOURAUD)["rgba"])
    shape, spacing = (30, 40, 50), (0.5, 0.5, 1.0)
    cam = V.camera_for_view("left", shape, spacing, (64, 48))
    mv = (m["verts"] + np.float32([12.0, -10.0, 14.0])).astype(np.float32)
    got = SV.render_surfaces([SV.SurfaceActor(mv, m["faces"], m["normals"])], "left", (64, 48), shape=shape, spacing=spacing)
    assert np.array_equal(got, R.render([R.layer(mv, m["faces"], m["normals"], SV.SURFACE_COLOUR[0])], cam)["rgba"]) and got[..., 3].any()
