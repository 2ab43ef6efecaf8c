"""Headless driver with an image filter: .inv3 -> --filter median 3 --threshold --stl --save.  The surface must be the
one made from the host-filtered image, and the saved project must carry the filtered version, its label and its meta."""
import json

import numpy as np
import pytest

from conftest import synth_volume

pytestmark = pytest.mark.gpu


def _run(capsys, argv):
    from invesalius3_amd import headless
    assert headless.main([str(a) for a in argv]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@pytest.mark.parametrize("two_d", [None, "coronal"])
def test_filter_threshold_stl_save(ivxlib, tmp_path, capsys, two_d):
    from invesalius3_amd import filters
    from invesalius3_amd import project as prj
    from invesalius3_amd import slice_
    img = synth_volume((30, 36, 44), seed=17)
    p = prj.Project(name="Synth", spacing=(0.5, 0.5, 1.0), threshold_range=(int(img.min()), int(img.max())))
    p.matrix = img
    src = tmp_path / "in.inv3"
    prj.save_inv3(src, p)
    dim, ori = ("3D", "Axial") if two_d is None else ("2D", two_d.capitalize())
    host = slice_.apply_image_filter(img, filters.MEDIAN, 3.0, dim, ori)
    assert not np.array_equal(host, img)
    # the same chain on a project whose image IS the host-filtered image, without --filter
    q = prj.Project(name="Synth", spacing=(0.5, 0.5, 1.0), threshold_range=(int(img.min()), int(img.max())))
    q.matrix = host
    pre = tmp_path / "pre.inv3"
    prj.save_inv3(pre, q)
    stl_a, stl_b, saved = tmp_path / "a.stl", tmp_path / "b.stl", tmp_path / "out.inv3"
    argv = [src, "--filter", "median", "3", "--threshold", 226, 3071, "--stl", stl_a, "--save", saved]
    if two_d:
        argv += ["--filter-2d", two_d]
    res = _run(capsys, argv)
    assert res["filter"] == {"type": "median", "value": 3.0, "dimension": dim, "orientation": ori}
    _run(capsys, [pre, "--threshold", 226, 3071, "--stl", stl_b])
    a, b = open(stl_a, "rb").read(), open(stl_b, "rb").read()
    assert len(a) > 84 and a[80:] == b[80:]
    r = prj.open_inv3(saved)
    try:
        assert [lbl for lbl, _m in r.image_versions] == ["original", "Filtered 1"]
        assert np.array_equal(r.image_versions[0][1], img) and np.array_equal(r.image_versions[1][1], host)
        assert np.array_equal(r.matrix, img)
        assert r.image_versions_meta == {"Filtered 1": {"applied_filter": "median", "sigma_smooth": "3.0", "derived": "original",
                                                        "dimension": dim, "orientation": ori}}
        assert r.masks[0].derived_from == "Filtered 1"
        want = np.where((host >= 226) & (host <= 3071), 255, 0).astype(np.uint8)
        assert np.array_equal(r.masks[0].interior, want)
    finally:
        r.close()
