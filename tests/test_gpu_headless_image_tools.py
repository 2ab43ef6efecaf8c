"""GPU: the headless driver's --flip, --swap-axes and --gantry-tilt: applied in that order before the threshold,
equal to the same steps done with numpy and live scipy, and recorded in the saved project with the new shape and spacing."""
import json

import numpy as np
import pytest

import _imagegeo_cases as C

pytestmark = pytest.mark.gpu


def test_headless_flip_swap_tilt_threshold_and_save(ivxlib, tmp_path, capsys):
    from invesalius3_amd import headless
    from invesalius3_amd import project as prj
    from invesalius3_amd import resident
    before = resident.count()
    img = C.disc_phantom((12, 20, 28), seed=31)
    spacing = (0.5, 0.75, 2.0)
    p = prj.Project(name="Synth", spacing=spacing, threshold_range=(int(img.min()), int(img.max())))
    p.matrix = img
    old = prj.new_mask(p, "old", (0, 100))  # a mask of the old shape: the swap recreates it empty
    old.matrix[:] = 255
    path, saved = tmp_path / "synth.inv3", tmp_path / "out.inv3"
    prj.save_inv3(path, p)
    lo, hi = 1000, 3071
    argv = [path, "--flip", 1, "--swap-axes", 2, 0, "--gantry-tilt", 5, "--threshold", lo, hi, "--save", saved]
    assert headless.main([str(a) for a in argv]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = np.array(img[:, ::-1].swapaxes(2, 0))
    want_spacing = (spacing[2], spacing[1], spacing[0])
    C.scipy_fix_gantry_tilt(want, want_spacing, 5)
    want_mask = np.where((want >= lo) & (want <= hi), 255, 0).astype(np.uint8)
    assert res["flip"] == 1 and res["swap_axes"] == [2, 0] and res["gantry_tilt"] == 5.0
    assert res["shape"] == list(want.shape) and res["spacing"] == list(want_spacing)
    assert res["mask_voxels"] == int((want_mask >= 127).sum()) > 0
    q = prj.open_inv3(saved)
    try:
        assert tuple(q.matrix_shape) == want.shape and tuple(q.spacing) == want_spacing
        assert np.array_equal(q.matrix, want)
        assert q.masks[0].matrix.shape == tuple(s + 1 for s in want.shape) and not q.masks[0].matrix.any()
        assert np.array_equal(q.masks[1].interior, want_mask)
    finally:
        q.close()
    assert resident.count() == before
