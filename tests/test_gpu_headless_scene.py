"""Headless driver with the 3-D scene: .inv3 -> --threshold --largest --render / --mask-preview composite --scene-png
--slice-planes.  The PNG must hold exactly what `scene3d.Scene3D.render` gives for the same field, surface and planes made by
hand with the Python calls, and the run's --png and --surface-png must be the bytes of a run without --scene-png."""
import json

import numpy as np
import pytest

import _scene3d_ref as R3
import _volren_ref as R

pytestmark = pytest.mark.gpu

SPACING = (0.5, 0.5, 1.0)
SIZE = (40, 32)
PRESETS, CLUTS, _ = R.fixture()
COLOUR, TRANSPARENCY, WINDOW = (1.0, 0.68, 0.33), 0.5, (1500.0, 100.0)
PLANES = (6, -1, 9)  # axial 6, no coronal plane, sagittal 9


def _run(capsys, argv):
    from invesalius3_amd import headless
    assert headless.main([str(a) for a in argv]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def _image():
    z, y, x = np.mgrid[:14, :18, :22]
    img = (-1000 + 40 * ((x + y + z) % 5)).astype(np.int16)
    img[(z - 6.5) ** 2 + (y - 8.5) ** 2 + (x - 8.5) ** 2 <= 5.0 ** 2] = 1000  # a ball ...
    img[(z - 6.5) ** 2 + (y - 8.5) ** 2 + (x - 18.0) ** 2 <= 2.0 ** 2] = 1200  # ... and a small one apart from it
    return img


@pytest.fixture(scope="module")
def case(ivxlib, tmp_path_factory):
    from invesalius3_amd import project as prj
    from invesalius3_amd import surface_process as sp
    from invesalius3_amd import volume as V
    img = _image()
    p = prj.Project(name="Balls", spacing=SPACING, threshold_range=(int(img.min()), int(img.max())))
    p.matrix = img
    tmp = tmp_path_factory.mktemp("scene")
    src = tmp / "in.inv3"
    prj.save_inv3(src, p)
    preset = tmp / "preset.plist"
    import plistlib
    with open(preset, "wb") as f:
        plistlib.dump(PRESETS["Bone + Skin"], f, fmt=plistlib.FMT_XML)
    mask = np.where((img >= 226) & (img <= 3071), 255, 0).astype(np.uint8)
    verts, faces = sp.marching_cubes_indexed(mask, SPACING, [127.0], 0, True, True, True, 0.0, 1)
    v1, f1, nreg = sp.keep_largest(verts, faces)
    assert nreg == 2
    assert not V.is_mip(PRESETS["Bone + Skin"]) and PRESETS["Bone + Skin"]["advancedCLUT"]  # (no colour list to look up)
    return {"src": src, "img": img, "mask": mask, "preset": preset, "largest": sp.point_normals(v1, f1)[:3]}


def _by_hand(case, field):
    """the scene of the run, made with the Python calls"""
    from invesalius3_amd import scene3d as S3
    from invesalius3_amd import slice_display as D
    from invesalius3_amd import surface_view as SV
    from invesalius3_amd.device import DeviceVolume
    pv, pf, pn = case["largest"]
    planes = [S3.SlicePlane(o, n) for o, n in zip(("AXIAL", "CORONAL", "SAGITAL"), PLANES) if n >= 0]
    state = D.DisplayState(window_width=WINDOW[0], window_level=WINDOW[1], mask_colour=(0.0, 1.0, 0.0))
    with DeviceVolume(case["img"], spacing=SPACING) as vol:
        vol.mask.upload(case["mask"])
        kw = {"preset": str(case["preset"])} if field == "image" else {"mask_colour": (0.0, 1.0, 0.0)}
        with S3.Scene3D(vol, [SV.SurfaceActor(pv, pf, pn, COLOUR, TRANSPARENCY)], planes) as sc:
            u8 = sc.render("left", SIZE, interpolation="phong", rgba8=True, state=state, **kw)
            f32 = sc.render("left", SIZE, interpolation="phong", state=state, **kw)
    return u8, f32


@pytest.mark.parametrize("field", ["image", "mask"])
def test_scene_png_equals_scene3d_render(case, tmp_path, capsys, field):
    from invesalius3_amd import volume as V
    png, scene, surf = tmp_path / "field.png", tmp_path / "scene.png", tmp_path / "surface.png"
    base = [case["src"], "--threshold", 226, 3071, "--largest", "--view", "left", "--size", *SIZE, "--png", png, "--surface-png", surf,
            "--surface-colour", *COLOUR, "--surface-transparency", TRANSPARENCY, "--surface-interpolation", "phong"]
    base += ["--render", case["preset"]] if field == "image" else ["--mask-preview", "composite"]
    _run(capsys, base)
    before = (V.read_png(str(png)), V.read_png(str(surf)))
    res = _run(capsys, base + ["--scene-png", scene, "--slice-planes", *PLANES, "--window", *WINDOW])
    assert res["scene"]["field"] == field and res["scene"]["planes"] == {"AXIAL": 6, "SAGITAL": 9}
    assert res["scene"]["triangles"] == len(case["largest"][1]) and res["scene"]["rays_hit"] > 0
    u8, f32 = _by_hand(case, field)
    got = V.read_png(str(scene))
    assert got.shape == (SIZE[1], SIZE[0], 4) and np.array_equal(got, u8) and np.array_equal(u8, R3.to_rgba8(f32))
    # the run's other pictures are what they were
    assert np.array_equal(V.read_png(str(png)), before[0]) and np.array_equal(V.read_png(str(surf)), before[1])
    # and the scene is neither of them: the planes and the translucent surface both show in it
    assert not np.array_equal(got, before[0]) and not np.array_equal(got, before[1])


def test_scene_png_argument_errors(case, tmp_path):
    from invesalius3_amd import headless
    for argv in ([case["src"], "--threshold", 226, 3071, "--slice-planes", 1, 1, 1],
                 [case["src"], "--threshold", 226, 3071, "--mask-preview", "iso", "--scene-png", tmp_path / "x.png"]):
        with pytest.raises(SystemExit):
            headless.main([str(a) for a in argv])
