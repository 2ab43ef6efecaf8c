"""The 3-D scene on the GPU (csrc/k_scene3d.hip) through libivx.so: every case of tests/_scene3d_cases.py against the
numpy restatement of rules S1 - S3 (tests/_scene3d_ref.py) within the ray casters' bound of 1e-3 on EVERY pixel, the exact
sample and ray counts next to it, and the equalities the rules promise bit for bit: a field alone is render_volume /
render_mask_preview, opaque surfaces alone are render_surfaces, skipping changes nothing, RGBA8 is the rounded float picture, two
renders and a shuffled triangle order give the same bytes.  Then the argument errors and what a re-render moves."""
import ctypes

import numpy as np
import pytest

import _scene3d_cases as C
import _scene3d_ref as R3
import _surface_view_cases as SC
import _surface_view_ref as SR

pytestmark = pytest.mark.gpu

TOL = 1e-3  # DESIGN 7d's bound on float32 sampling against the float64 restatement
CASES = {c["name"]: c for c in C.cases()}
MAX_ERR = {}


@pytest.fixture(scope="module")
def mods(ivxlib):
    from invesalius3_amd import scene3d, surface_view
    return scene3d, surface_view


@pytest.fixture(scope="module")
def volumes(ivxlib):
    """one DeviceVolume per (volume, spacing); the small one carries the mask matrix's interior"""
    from invesalius3_amd.device import DeviceVolume
    made = {}

    def get(which, spacing=C.SPACING):
        key = (which, tuple(spacing))
        if key not in made:
            v = made[key] = DeviceVolume(np.array(C.image(which)), spacing=spacing)
            if which == "small":
                v.mask.upload_view(C.mask_matrix()[1:, 1:, 1:])
        return made[key]

    yield get
    for v in made.values():
        v.close()


def actors_of(SV, layers):
    return [SV.SurfaceActor(m["verts"], m["faces"], m["normals"], m["colour"], m["transparency"]) for m in layers]


def scene_of(mods, volumes, case, layers=None):
    S3, SV = mods
    vol = volumes(case["which"], case["spacing"]) if case["kind"] != R3.NONE else None
    planes = [S3.SlicePlane(p["orientation"], p["n"], p["picture"], p["opacity"]) for p in case["planes"]]
    layers = case["layers"] if layers is None else layers
    return S3.Scene3D(vol, actors_of(SV, layers) if layers else None, planes, spacing=case["spacing"])


def render_args(case, **kw):
    args = dict(camera=case["cam"], size=case["size"], interpolation=case["mode"], sample_distance=case["dt"])
    if case["kind"] == R3.IMAGE:
        args.update(preset=case["preset"], clip_plane=case["clip"], shade=case["shade"], color_lists=C.CLUTS)
    elif case["kind"] == R3.MASK:
        args.update(mask_colour=case["colour"], background=C.BACKGROUND)
    else:
        args.update(background=C.BACKGROUND)
    args.update(kw)
    return args


# ---- 1: every case against the restatement, with the equalities that pin the order ------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_the_restatement(mods, volumes, name):
    case = CASES[name]
    ref = C.reference(case)
    w, h = case["size"]
    with scene_of(mods, volumes, case) as sc:
        off = sc.render(**render_args(case, skip=False))
        st_off = dict(sc.last_render_stats)
        on = sc.render(**render_args(case, skip=True))
        st_on = dict(sc.last_render_stats)
        again = sc.render(**render_args(case, skip=True))
        u8 = sc.render(**render_args(case, skip=True, rgba8=True))
    assert off.shape == (h, w, 4) and off.dtype == np.float32
    err = np.abs(off.astype(np.float64) - ref["image"])
    MAX_ERR[name] = float(err.max())
    print("scene3d %-36s max deviation %.3g" % (name, err.max()))
    assert err.max() <= TOL, "max error %.3g at pixel %r" % (err.max(), np.unravel_index(err.max(-1).argmax(), (h, w)))
    # the sample counts are exact: a fragment one sample early or late would show here
    assert st_off["samples"] == int(ref["taken"].sum()) and st_off["skipped"] == 0
    assert st_off["rays_hit"] == int(ref["hit"].sum()) and st_off["early"] == int(ref["early"].sum())
    # skipping changes no bit and no count
    assert on.tobytes() == off.tobytes()
    assert st_on["samples"] + st_on["skipped"] == st_off["samples"]
    assert (st_on["early"], st_on["rays_hit"]) == (st_off["early"], st_off["rays_hit"])
    assert again.tobytes() == on.tobytes()
    assert u8.dtype == np.uint8 and np.array_equal(u8, R3.to_rgba8(on))  # (write_pixel rounds in float32)


def test_skipping_skips_and_fragments_cap_the_jumps(mods, volumes):
    """the 20 x 24 x 28 field under the Standard preset has empty macro cells with the quad and the planes inside them: jumps
    happen, and fragments lie strictly inside some (test_case_equals_the_restatement shows that they end at K_f: no bit and no
    count changes)"""
    case = CASES["cells iso skipping"]
    assert C.capped_jumps(case) > 50
    with scene_of(mods, volumes, case) as sc:
        sc.render(**render_args(case, skip=True))
        print("scene3d skipped samples", sc.last_render_stats)
        assert sc.last_render_stats["skipped"] > 1000


def test_the_termination_cases_show_what_they_are_for(mods, volumes):
    S3, SV = mods
    with scene_of(mods, volumes, CASES["nothing anywhere"]) as sc:
        got = sc.render(**render_args(CASES["nothing anywhere"]))
        assert (got == np.array(C.BACKGROUND + (0.0,), np.float32)).all()
    case = CASES["opaque surface in front"]
    covered = SR.raster_keys(case["layers"][0]["verts"], case["layers"][0]["faces"], case["cam"]) != SR.EMPTY
    assert covered.all()
    with scene_of(mods, volumes, case) as sc:
        got = sc.render(**render_args(case))
        assert sc.last_render_stats["samples"] == 0 and sc.last_render_stats["early"] == covered.size
        alone = SV.render_surfaces(actors_of(SV, case["layers"]), case["cam"], case["size"])
        assert got.tobytes() == alone.tobytes() and (got[..., 3] == 1.0).all()  # nothing of the field shows
    case = CASES["opaque preset hides the surface"]
    vol = volumes("small")
    with scene_of(mods, volumes, case) as sc:
        assert sc.render(**render_args(case)).tobytes() == vol.render_volume(case["preset"], case["cam"], case["size"], color_lists=C.CLUTS).tobytes()
    case = CASES["clip plane"]
    with scene_of(mods, volumes, case) as sc:
        clipped, whole = sc.render(**render_args(case)), sc.render(**render_args(case, clip_plane=None))
        alone = SV.render_surfaces(actors_of(SV, case["layers"]), case["cam"], case["size"])
    assert not np.array_equal(clipped, whole)
    # where the clip plane removed the field in front of the sphere, the sphere shows as it is: it is not clipped
    ref = C.reference(case)
    bare = (ref["kf"][0].reshape(alone.shape[:2]) == 0) & (alone[..., 3] == 1.0)
    assert bare.sum() > 5 and np.array_equal(clipped[bare], alone[bare])
    case = CASES["eleven fragments"]
    assert (C.reference(case)["order"] >= 0).all(axis=0).any()  # a pixel with all eleven


# ---- 2: the parts alone, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,size", [("small", (19, 13)), ("cells", (64, 48))])
def test_field_alone_is_render_volume(mods, volumes, which, size):
    S3, _ = mods
    vol = volumes(which)
    with S3.Scene3D(vol) as sc:
        for name, view, shade in (("Bone + Skin", "iso", True), ("Gold Bone", "front", True), ("Standard", "top", None)):
            want = vol.render_volume(C.PRESETS[name], view, size, shade=shade, color_lists=C.CLUTS)
            st = dict(vol.last_render_stats)
            got = sc.render(view, size, preset=C.PRESETS[name], shade=shade, color_lists=C.CLUTS)
            assert got.tobytes() == want.tobytes(), (name, view)
            assert sc.last_render_stats == st
            assert vol.render_scene(view, size, preset=C.PRESETS[name], shade=shade, color_lists=C.CLUTS).tobytes() == want.tobytes()
    b = np.array([0.0, 0.0, 0.0])
    n = np.array([0.0, 0.6, 0.8])
    with S3.Scene3D(vol) as sc:
        from invesalius3_amd import volume as V
        bb = V.volume_bounds(vol.shape, vol.spacing)
        b = np.array([(bb[0] + bb[1]) / 2, (bb[2] + bb[3]) / 2, (bb[4] + bb[5]) / 2])
        want = vol.render_volume(C.PRESETS["Bone + Skin"], "iso", size, clip_plane=(n, b), color_lists=C.CLUTS)
        assert sc.render("iso", size, preset=C.PRESETS["Bone + Skin"], clip_plane=(n, b), color_lists=C.CLUTS).tobytes() == want.tobytes()


def test_field_alone_is_the_composite_mask_preview(mods, volumes):
    S3, _ = mods
    vol = volumes("small")
    with S3.Scene3D(vol) as sc:
        for view, size in (("iso", (19, 13)), ("front", (64, 48)), ("top", (19, 13))):
            want = vol.render_mask_preview((0.9, 0.8, 0.2), view, size, background=C.BACKGROUND)
            st = dict(vol.last_render_stats)
            got = sc.render(view, size, mask_colour=(0.9, 0.8, 0.2), background=C.BACKGROUND)
            assert got.tobytes() == want.tobytes(), view
            assert sc.last_render_stats == st


SURFACE_SCENES = {s["name"]: s for s in SC.scenes()}


@pytest.mark.parametrize("name", ["icosphere iso", "icosphere top", "cube 256", "degenerate", "viewport 257 x 3", "no surface"])
def test_opaque_surfaces_alone_are_render_surfaces(mods, name):
    S3, SV = mods
    s = SURFACE_SCENES[name]
    layers = [dict(m, transparency=0.0, opacity=np.float32(1.0)) for m in s["layers"]]
    size = s["cam"]["viewport"]
    for mode in (SR.FLAT, SR.GOURAUD, SR.PHONG):
        want = SV.render_surfaces(actors_of(SV, layers), s["cam"], size, interpolation=mode, background=C.BACKGROUND)
        with S3.Scene3D(None, actors_of(SV, layers) if layers else None) as sc:
            got = sc.render(s["cam"], size, interpolation=mode, background=C.BACKGROUND)
        assert got.tobytes() == want.tobytes(), (name, mode)


def test_host_form_equals_the_resident_form(mods, volumes):
    S3, SV = mods
    for name in ("small iso scene", "mask field", "surfaces and planes alone"):
        case = CASES[name]
        with scene_of(mods, volumes, case) as sc:
            want = sc.render(**render_args(case))
        kw = render_args(case)
        planes = [S3.SlicePlane(p["orientation"], p["n"], p["picture"], p["opacity"]) for p in case["planes"]]
        if case["kind"] == R3.IMAGE:
            kw["image"] = np.array(C.image(case["which"]))
        elif case["kind"] == R3.MASK:
            kw["mask"] = np.array(C.mask_matrix())
        got = S3.render_scene(spacing=case["spacing"], actors=actors_of(SV, case["layers"]), planes=planes, shape=case["shape"], **kw)
        assert got.tobytes() == want.tobytes(), name


def test_shuffled_triangle_order_gives_the_same_picture(mods, volumes):
    case = CASES["small iso scene"]
    rng = np.random.default_rng(11)
    shuffled = [dict(m, faces=np.ascontiguousarray(m["faces"][rng.permutation(len(m["faces"]))])) for m in case["layers"]]
    with scene_of(mods, volumes, case) as a, scene_of(mods, volumes, case, shuffled) as b:
        assert a.render(**render_args(case)).tobytes() == b.render(**render_args(case)).tobytes()


# ---- 3: argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors(mods, volumes, ivxlib):
    S3, SV = mods
    L = ivxlib
    vol = volumes("small")
    case = CASES["small iso scene"]
    nine = actors_of(SV, SC.eight_layers(9))
    with S3.Scene3D(vol, nine) as sc:
        with pytest.raises(ValueError):
            sc.render("iso", (16, 16))
    shape = C.SHAPES["small"]
    four = [S3.SlicePlane(o, 1, C.slice_picture(o, shape)) for o in ("AXIAL", "CORONAL", "SAGITAL", "AXIAL")]
    with S3.Scene3D(vol, None, four) as sc:
        with pytest.raises(ValueError):
            sc.render("iso", (16, 16))
    with S3.Scene3D(vol, None, four[2:]) as sc:  # SAGITAL, AXIAL
        sc.render("iso", (16, 16))
        sc.planes = [four[0], four[3]]            # AXIAL twice
        with pytest.raises(ValueError):
            sc.render("iso", (16, 16))
    with S3.Scene3D(vol) as sc:
        with pytest.raises(ValueError):
            sc.render("iso", (16, 16), preset=C.PRESETS["MIP"], color_lists=C.CLUTS)
        with pytest.raises(ValueError):
            sc.render("iso", (16, 16), mask_colour=(1.0, 0.0, 0.0), mask_mode="iso")
        with pytest.raises(ValueError):
            sc.render("iso", (16, 16), preset=C.PRESETS["Standard"], mask_colour=(1.0, 0.0, 0.0), color_lists=C.CLUTS)
    # the C ABI says IVX_EINVAL before anything is launched
    from invesalius3_amd import volume as V
    cam = SC.hand_cam()
    setup = S3.field_setup(dict(cam, **{k: np.asarray(cam[k], np.float64) for k in ("focal", "right", "up", "dir")}), (1.0, 1.0, 1.0))[1]
    p, cc = V.volren_params(setup, (1.0, 1.0, 1.0)), SV._c_camera(cam)
    out = np.zeros((16, 16, 4), np.float32)
    layers, planes = (SV.SurfaceLayer * 9)(), (S3.ScenePlane * 4)()
    pic = C.slice_picture("AXIAL", shape)
    for k, m in enumerate(planes):
        m.picture, m.h, m.w, m.orientation, m.opacity = pic.ctypes.data, pic.shape[0], pic.shape[1], k % 3, 1.0

    def dev(nlayers=0, nplanes=0, params=p, camera=cc, pl=planes):
        return L.lib().ivx_dev_scene_render(0, None, None, None, None, 0, 0, None, None, layers, nlayers, ctypes.byref(camera), 1, pl, nplanes,
                                            ctypes.byref(params), L.ptr(out), None, None)

    def host(nlayers=0, nplanes=0, params=p):
        return L.lib().ivx_scene_render(0, None, None, None, 0, 0, None, None, layers, nlayers, ctypes.byref(cc), 1, planes, nplanes,
                                        ctypes.byref(params), L.ptr(out))

    assert dev(nlayers=9) == L.IVX_EINVAL and host(nlayers=9) == L.IVX_EINVAL
    assert dev(nplanes=4) == L.IVX_EINVAL and host(nplanes=4) == L.IVX_EINVAL
    twice = (S3.ScenePlane * 4)()
    for k, m in enumerate(twice):
        m.picture, m.h, m.w, m.orientation, m.opacity = pic.ctypes.data, pic.shape[0], pic.shape[1], 0, 1.0
    assert dev(nplanes=2, pl=twice) == L.IVX_EINVAL
    mip = V.volren_params(dict(setup, mip=True), (1.0, 1.0, 1.0))
    assert dev(params=mip) == L.IVX_EINVAL and host(params=mip) == L.IVX_EINVAL
    other = SV._c_camera(SC.hand_cam((16, 8)))
    assert dev(camera=other) == L.IVX_EINVAL


# ---- 4: what a re-render moves ------------------------------------------------------------------------------------------------------
def test_a_rerender_uploads_tables_only_and_rasters_only_for_a_new_camera(mods, volumes):
    S3, SV = mods
    from invesalius3_amd import resident, slice_display as D, volume as V
    vol = volumes("cells")
    case = CASES["cells iso scene"]
    size = case["size"]
    actors = actors_of(SV, case["layers"])
    planes = [S3.SlicePlane(o, n) for o, n in (("AXIAL", 5), ("CORONAL", 6), ("SAGITAL", 7))]  # the volume's own slice pictures
    state = D.DisplayState(window_width=2000.0, window_level=300.0)
    kw = dict(camera="iso", size=size, preset=C.PRESETS["Bone + Skin"], color_lists=C.CLUTS, state=state)
    picture = size[0] * size[1] * 16
    # the slice display's byte tables: what one default plane picture uploads
    show = 3 * D.build(state, D.IMG_I16, D.ST_ALL, image_range=vol._image_min_max(), have_mask=False, aux_colours=None)[1].nbytes

    def moved(fn):
        before = resident.transfer_stats()
        out = fn()
        after = resident.transfer_stats()
        return out, after["h2d_bytes"] - before["h2d_bytes"], after["d2h_bytes"] - before["d2h_bytes"]

    with S3.Scene3D(vol, actors, planes) as sc:
        first = sc.render(**kw)
        runs = sc.surfaces.raster_runs
        assert runs == len(actors)
        # colour and transparency: kernel arguments
        actors[0].colour, actors[1].transparency = C.BLUE, 0.25
        a, up, down = moved(lambda: sc.render(**kw))
        assert not np.array_equal(a, first) and sc.surfaces.raster_runs == runs
        assert up == show and picture <= down <= picture + 64  # (the counters and the image's range come down too)
        # window / level of the planes, a plane's slice
        state.window_level = 100.0
        planes[0].n = 9
        b, up, down = moved(lambda: sc.render(**kw))
        assert not np.array_equal(a, b) and sc.surfaces.raster_runs == runs
        assert up == show and picture <= down <= picture + 64
        # the preset's window: the baked table goes up, and nothing else
        p2 = V.set_wwwl(C.PRESETS["Bone + Skin"], 300.0, 200.0, 0)
        setup = V.render_setup(p2, (int(C.image("cells").min()), int(C.image("cells").max())), case["cam"], color_lists=C.CLUTS)
        table = sum(t.nbytes for t in (V.device_tables(setup)[0], V.device_tables(setup)[2]))
        c, up, down = moved(lambda: sc.render(**dict(kw, preset=p2)))
        assert not np.array_equal(b, c) and sc.surfaces.raster_runs == runs
        assert up == table + show and picture <= down <= picture + 64
        # a new camera rasters every surface again, and still uploads no mesh
        d, up, down = moved(lambda: sc.render(**dict(kw, preset=p2, camera="front")))
        assert sc.surfaces.raster_runs == runs + len(actors) and up == show
        # and the pictures are those of a fresh scene
        with S3.Scene3D(vol, actors_of(SV, case["layers"]), [S3.SlicePlane(o, n) for o, n in (("AXIAL", 9), ("CORONAL", 6), ("SAGITAL", 7))]) as fresh:
            fa = fresh.surfaces.actors
            fa[0].colour, fa[1].transparency = C.BLUE, 0.25
            assert fresh.render(**dict(kw, preset=p2, camera="front")).tobytes() == d.tobytes()


def test_default_plane_pictures_are_show_slice(mods, volumes):
    """a plane without a picture shows DeviceVolume.show_slice's bytes of its slice"""
    S3, _ = mods
    from invesalius3_amd import slice_display as D
    vol = volumes("small")
    state = D.DisplayState(window_width=1500.0, window_level=200.0)
    shape = C.SHAPES["small"]
    spec = (("AXIAL", 4), ("CORONAL", 3), ("SAGITAL", 6))
    pictures = [vol.show_slice(o, n, state, mask=False) for o, n in spec]
    for pic, (o, n) in zip(pictures, spec):
        assert pic.shape == S3.plane_shape(o, shape) + (3,)
    with S3.Scene3D(vol, None, [S3.SlicePlane(o, n) for o, n in spec]) as a, \
            S3.Scene3D(vol, None, [S3.SlicePlane(o, n, pic) for (o, n), pic in zip(spec, pictures)]) as b:
        got = a.render("iso", (19, 13), state=state)
        assert got.tobytes() == b.render("iso", (19, 13)).tobytes()
        assert (got[..., 3] == 1.0).sum() > 20
