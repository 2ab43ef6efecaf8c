"""Headless driver with --mask-preview: the PNG it writes decodes to DeviceVolume.render_mask_preview's pixels, and
--render together with --mask-preview is an error."""
import json

import numpy as np
import pytest

import _volren_ref as R

pytestmark = pytest.mark.gpu


def _project(tmp_path):
    from invesalius3_amd import project as prj
    img = R.cropped_ct((30, 36, 40), seed=9)
    spacing = (0.8, 0.8, 1.2)
    p = prj.Project(name="Synth", spacing=spacing, threshold_range=(int(img.min()), int(img.max())))
    p.matrix = img
    src = tmp_path / "in.inv3"
    prj.save_inv3(src, p)
    return src, img, spacing


@pytest.mark.parametrize("mode,view,colour", [("iso", "iso", None), ("composite", "front", (0.9, 0.3, 0.1))])
def test_mask_preview_png(ivxlib, tmp_path, capsys, mode, view, colour):
    from invesalius3_amd import headless
    from invesalius3_amd import volume as V
    from invesalius3_amd.device import DeviceVolume
    src, img, spacing = _project(tmp_path)
    png = tmp_path / "mask.png"
    argv = [src, "--threshold", 226, 3071, "--mask-preview", mode, "--view", view, "--size", 64, 48, "--png", png]
    if colour is not None:
        argv += ["--mask-colour", *colour]
    assert headless.main([str(a) for a in argv]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["mask_preview"]["png"] == str(png) and out["mask_preview"]["mode"] == mode
    assert out["mask_preview"]["size"] == [64, 48] and out["mask_preview"]["rays_hit"] > 0 and "mask_preview" in out["gpu_ms"]
    assert out["threshold"] == [226, 3071] and out["mask_voxels"] > 0
    got = V.read_png(str(png))
    with DeviceVolume(img, spacing=spacing) as v:
        v.threshold(226, 3071)
        ref = v.render_mask_preview((0.0, 1.0, 0.0) if colour is None else colour, view, (64, 48), mode=mode, rgba8=True)
    assert got.shape == (48, 64, 4) and np.array_equal(got, ref)
    assert np.count_nonzero(got[..., 3] == 255) > 100  # the bone is there


def test_render_and_mask_preview_together_are_an_error(ivxlib, tmp_path, capsys):
    from invesalius3_amd import headless
    src, _, _ = _project(tmp_path)
    with pytest.raises(SystemExit) as e:
        headless.main([str(src), "--threshold", "226", "3071", "--render", "x.plist", "--mask-preview", "iso"])
    assert e.value.code == 2
    assert "--mask-preview" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        headless.main([str(src), "--png", str(tmp_path / "a.png")])
