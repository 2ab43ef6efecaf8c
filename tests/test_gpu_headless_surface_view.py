"""Headless driver with the surface view: .inv3 -> --threshold --largest --surface-png.  The PNG must hold exactly
`volume.to_rgba8` of `surface_view.render_surfaces` on the mesh of the same chain made by hand with the Python calls, under the
camera of the image, for every interpolation name, with and without --stl."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPACING = (0.5, 0.5, 1.0)
SIZE = (72, 56)


def _run(capsys, argv):
    from invesalius3_amd import headless
    assert headless.main([str(a) for a in argv]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def _image():
    z, y, x = np.mgrid[:26, :26, :40]
    img = np.full(z.shape, -1000, np.int16)
    img[(z - 12.5) ** 2 + (y - 12.5) ** 2 + (x - 12.5) ** 2 <= 10.0 ** 2] = 1000  # a ball ...
    img[(z - 12.5) ** 2 + (y - 12.5) ** 2 + (x - 32.5) ** 2 <= 4.0 ** 2] = 1200   # ... and a small one apart from it
    return img


@pytest.fixture(scope="module")
def case(ivxlib, tmp_path_factory):
    from invesalius3_amd import project as prj
    from invesalius3_amd import surface_process as sp
    img = _image()
    p = prj.Project(name="Balls", spacing=SPACING, threshold_range=(int(img.min()), int(img.max())))
    p.matrix = img
    src = tmp_path_factory.mktemp("surface_view") / "in.inv3"
    prj.save_inv3(src, p)
    mask = np.where((img >= 226) & (img <= 3071), 255, 0).astype(np.uint8)
    verts, faces = sp.marching_cubes_indexed(mask, SPACING, [127.0], 0, True, True, True, 0.0, 1)
    v1, f1, nreg = sp.keep_largest(verts, faces)
    assert nreg == 2
    return {"src": src, "shape": img.shape, "all": sp.point_normals(verts, faces)[:3], "largest": sp.point_normals(v1, f1)[:3]}


@pytest.mark.parametrize("name", ["flat", "gouraud", "phong"])
def test_surface_png_equals_render_surfaces(case, tmp_path, capsys, name):
    from invesalius3_amd import surface_view as SV
    from invesalius3_amd import volume as V
    colour, transparency = (1.0, 0.68, 0.33), 0.25
    for with_stl in (False, True):
        png = tmp_path / ("%s_%d.png" % (name, with_stl))
        argv = [case["src"], "--threshold", 226, 3071, "--largest", "--view", "left", "--size", *SIZE, "--surface-png", png,
                "--surface-colour", *colour, "--surface-transparency", transparency, "--surface-interpolation", name]
        res = _run(capsys, argv + (["--stl", tmp_path / "out.stl"] if with_stl else []))
        pv, pf, pn = case["largest"]
        assert res["surface_view"]["triangles"] == len(pf) and res["surface_view"]["interpolation"] == name and ("stl" in res) == with_stl
        want = SV.render_surfaces([SV.SurfaceActor(pv, pf, pn, colour, transparency)], "left", SIZE, shape=case["shape"], spacing=SPACING,
                                  interpolation=name)
        got = V.read_png(str(png))
        assert got.shape == (SIZE[1], SIZE[0], 4) and np.array_equal(got, V.to_rgba8(want))
        assert (got[..., 3] == 191).any() and (got[..., 3] == 0).any()  # the ball, 0.75 opaque, and the background around it


def test_surface_png_defaults_and_the_whole_surface(case, tmp_path, capsys):
    from invesalius3_amd import surface_view as SV
    from invesalius3_amd import volume as V
    png = tmp_path / "all.png"
    res = _run(capsys, [case["src"], "--threshold", 226, 3071, "--size", *SIZE, "--surface-png", png])
    pv, pf, pn = case["all"]
    assert res["surface_view"]["view"] == "iso" and res["surface_view"]["colour"] == [0.33, 1.0, 0.33]
    want = SV.render_surfaces([SV.SurfaceActor(pv, pf, pn)], "iso", SIZE, shape=case["shape"], spacing=SPACING, rgba8=True)
    assert np.array_equal(V.read_png(str(png)), want) and np.array_equal(want, V.to_rgba8(
        SV.render_surfaces([SV.SurfaceActor(pv, pf, pn)], "iso", SIZE, shape=case["shape"], spacing=SPACING)))
    assert (want[..., 3] == 255).sum() > 200
