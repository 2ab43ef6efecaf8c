"""GPU: DeviceVolume.cut_mask / brush_mask_stroke and the headless --cut-polygon / --brush3d against the module functions of
invesalius3_amd/mask3d_editor.py on a tiny .inv3."""
import json

import numpy as np
import pytest

from invesalius3_amd import mask3d_editor as M3
from invesalius3_amd import volume as V
from invesalius3_amd.device import DeviceVolume

pytestmark = pytest.mark.gpu
SPACING = (0.5, 0.5, 1.0)
SIZE = (96, 64)
POLYGON = [20.5, 10.0, 80.0, 14.5, 60.0, 55.0, 30.0, 50.0]
DABS = [3.0, -2.0, 3.0, 4.0, -3.0, 4.0, 5.5, -4.5, 5.0, 40.0, -2.0, 3.0]


def expected(img, lo, hi, cuts, strokes, view="iso"):
    """the module functions on the padded host matrix: (matrix, slices changed per cut, per stroke)"""
    m = np.zeros(tuple(s + 1 for s in img.shape), np.uint8)
    m[1:, 1:, 1:] = np.where((img >= lo) & (img <= hi), 255, 0)
    cam = V.resolve_camera(view, img.shape, SPACING, SIZE)
    near, far = M3.default_clipping_range(cam)
    wts, wtc = M3.camera_matrices(cam, SIZE, (near, far))
    nc, ns = [], []
    for mode, depth, pts in cuts:
        nc.append(M3.cut_mask(m, SPACING, [np.asarray(pts, np.float64).reshape(-1, 2)], SIZE, wts, wtc, near + (far - near) * depth, mode))
    for mode, size, pts in strokes:
        ns.append(M3.brush_stroke(m, None, SPACING, np.asarray(pts, np.float64).reshape(-1, 3), size, mode))
    return m, nc, ns


def test_device_volume_cut_and_stroke(ivxlib):
    from conftest import synth_volume
    img = synth_volume((12, 20, 28), seed=31)
    lo, hi = max(int(np.median(img)) + 800, 0), 3071
    cuts, strokes = [(1, 1.0, POLYGON), (0, 0.6, POLYGON)], [(1, 4.0, DABS), (0, 3.0, DABS[:6])]
    want, nc, ns = expected(img, lo, hi, cuts, strokes)
    cam = V.resolve_camera("iso", img.shape, SPACING, SIZE)
    near, far = M3.default_clipping_range(cam)
    wts, wtc = M3.camera_matrices(cam, SIZE, (near, far))
    with DeviceVolume(img, spacing=SPACING) as vol:
        vol.threshold(lo, hi)
        before = vol.download_mask().copy()
        assert (before == 255).any()
        for (mode, depth, pts), n in zip(cuts, nc):
            flags = vol.cut_mask([np.asarray(pts).reshape(-1, 2)], SIZE, wts, wtc, near + (far - near) * depth, mode)
            after = vol.download_mask().copy()
            assert np.array_equal(flags, (before != after).any(axis=(1, 2))) and int(flags.sum()) == n
            before = after
        for (mode, size, pts), n in zip(strokes, ns):
            flags = vol.brush_mask_stroke(np.asarray(pts).reshape(-1, 3), size, mode)
            after = vol.download_mask().copy()
            assert np.array_equal(flags, (before != after).any(axis=(1, 2))) and int(flags.sum()) == n
            before = after
        assert np.array_equal(before, want[1:, 1:, 1:])
        assert sum(nc) > 0 and sum(ns) > 0
        # the planes the pipeline keeps of the mask went with the write: a fresh threshold gives the fresh mask again
        vol.threshold(lo, hi)
        assert np.array_equal(vol.download_mask(), np.where((img >= lo) & (img <= hi), 255, 0))


def test_headless_cut_polygon_and_brush3d(ivxlib, tmp_path, capsys):
    from conftest import synth_volume
    from invesalius3_amd import headless
    from invesalius3_amd import project as prj
    img = synth_volume((12, 20, 28), seed=31)
    p = prj.Project(name="Synth", spacing=SPACING, threshold_range=(int(img.min()), int(img.max())))
    p.matrix = img
    path, saved = tmp_path / "synth.inv3", tmp_path / "out.inv3"
    prj.save_inv3(path, p)
    lo, hi = max(int(np.median(img)) + 800, 0), 3071
    argv = [path, "--threshold", lo, hi, "--view", "iso", "--cut-size", *SIZE, "--cut-polygon", 1, 1.0, *POLYGON, "--cut-polygon", 0, 0.6, *POLYGON,
            "--brush3d", 0, 4.0, *DABS, "--save", saved]
    assert headless.main([str(a) for a in argv]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want, nc, ns = expected(img, lo, hi, [(1, 1.0, POLYGON), (0, 0.6, POLYGON)], [(0, 4.0, DABS)])
    assert [c["slices_changed"] for c in res["cut_polygon"]] == nc and [b["slices_changed"] for b in res["brush3d"]] == ns
    assert sum(nc) > 0 and sum(ns) > 0
    assert res["mask_voxels"] == int((want[1:, 1:, 1:] >= 127).sum()) > 0
    q = prj.open_inv3(saved)
    try:
        assert np.array_equal(q.masks[0].interior, want[1:, 1:, 1:])
    finally:
        q.close()
