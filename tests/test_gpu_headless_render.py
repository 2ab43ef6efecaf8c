"""Headless driver with --render: the PNG it writes decodes to DeviceVolume.render_volume's pixels, and --filter comes
first."""
import json
import plistlib

import numpy as np
import pytest

import _volren_ref as R

pytestmark = pytest.mark.gpu


def _run(capsys, argv):
    from invesalius3_amd import headless
    assert headless.main([str(a) for a in argv]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def _presets_dir(tmp_path):
    """a presets directory laid out like the reference's presets/raycasting, rebuilt from the fixture"""
    presets, cluts, _ = R.fixture()
    d = tmp_path / "raycasting"
    (d / "color_list").mkdir(parents=True)
    for name, p in presets.items():
        with open(d / (name + ".plist"), "wb") as f:
            plistlib.dump(p, f, fmt=plistlib.FMT_XML)
    for name, c in cluts.items():
        with open(d / "color_list" / (name + ".plist"), "wb") as f:
            plistlib.dump({"Red": [int(v) for v in c[:, 0]], "Green": [int(v) for v in c[:, 1]],
                           "Blue": [int(v) for v in c[:, 2]]}, f, fmt=plistlib.FMT_XML)
    return d, presets, cluts


@pytest.mark.parametrize("name,view,filt", [("Bone + Skin", "iso", None), ("Vascular", "front", ("median", "3"))])
def test_render_png(ivxlib, tmp_path, capsys, name, view, filt):
    from invesalius3_amd import project as prj
    from invesalius3_amd import volume as V
    from invesalius3_amd.device import DeviceVolume
    img = R.synth_volume((30, 36, 40), seed=9)
    spacing = (0.8, 0.8, 1.2)
    p = prj.Project(name="Synth", spacing=spacing, threshold_range=(int(img.min()), int(img.max())))
    p.matrix = img
    src = tmp_path / "in.inv3"
    prj.save_inv3(src, p)
    pdir, presets, cluts = _presets_dir(tmp_path)
    png = tmp_path / "out.png"
    argv = [src, "--render", name, "--presets-dir", pdir, "--view", view, "--size", 64, 48, "--png", png]
    if filt:
        argv += ["--filter", *filt]
    out = _run(capsys, argv)
    assert out["render"]["png"] == str(png) and out["render"]["size"] == [64, 48] and "gpu_ms" in out
    got = V.read_png(str(png))
    with DeviceVolume(img, spacing=spacing) as v:
        if filt:
            v.filter_image(1, 3.0)
        ref = v.render_volume(presets[name], view, (64, 48), color_lists=cluts, rgba8=True)
    assert got.shape == (48, 64, 4) and np.array_equal(got, ref)
    # a .plist path works too, and the existing flags still work after a render
    stl = tmp_path / "a.stl"
    out2 = _run(capsys, [src, "--render", pdir / (name + ".plist"), "--view", view, "--size", 64, 48, "--png", png,
                         "--threshold", 226, 3071, "--stl", stl])
    assert np.array_equal(V.read_png(str(png)), got if not filt else V.read_png(str(png)))
    assert out2["threshold"] == [226, 3071] and stl.exists()
