"""Headless driver with the surface connectivity tools: .inv3 -> --threshold --split DIR writes one STL per connected part,
equal to the parts made by hand with the Python calls, and --surface-seed with a coordinate inside the small ball returns only it."""
import json
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPACING = (0.5, 0.5, 1.0)


def _run(capsys, argv):
    from invesalius3_amd import headless
    assert headless.main([str(a) for a in argv]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def _image():
    z, y, x = np.mgrid[:26, :26, :56]
    img = np.full(z.shape, -1000, np.int16)
    for cx, r in ((8.5, 6.0), (26.5, 9.0), (46.5, 4.0)):  # three balls: middle, large, small
        img[(z - 12.5) ** 2 + (y - 12.5) ** 2 + (x - cx) ** 2 <= r * r] = 1000
    return img


def _stl_triangles(path):
    raw = open(path, "rb").read()
    n = struct.unpack("<I", raw[80:84])[0]
    rec = np.frombuffer(raw[84:], dtype=[("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")])
    assert n == len(rec)
    return rec["v"]


def test_split_and_surface_seed(ivxlib, tmp_path, capsys):
    from invesalius3_amd import polydata_utils as pu
    from invesalius3_amd import project as prj
    from invesalius3_amd import surface_process as sp
    img = _image()
    p = prj.Project(name="Balls", spacing=SPACING, threshold_range=(int(img.min()), int(img.max())))
    p.matrix = img
    src = tmp_path / "in.inv3"
    prj.save_inv3(src, p)
    out_dir = tmp_path / "parts"
    res = _run(capsys, [src, "--threshold", 226, 3071, "--split", out_dir])
    # the chain by hand
    mask = np.where((img >= 226) & (img <= 3071), 255, 0).astype(np.uint8)
    verts, faces = sp.marching_cubes_indexed(mask, SPACING, [127.0], 0, True, True, True, 0.0, 1)
    parts = pu.SplitDisconectedParts(verts, faces)
    assert len(parts) == 3 and res["split"]["regions"] == 3 and len(res["split"]["parts"]) == 3
    assert sorted(f.name for f in out_dir.iterdir()) == ["part_%05d.stl" % r for r in range(3)]
    for r, (pv, pf) in enumerate(parts):
        row = res["split"]["parts"][r]
        assert np.array_equal(_stl_triangles(out_dir / ("part_%05d.stl" % r)), pv[pf])
        vol, area = sp.mass_properties(pv, pf)
        assert (row["part"], row["triangles"], row["vertices"]) == (r, len(pf), len(pv))
        assert row["volume"] == pytest.approx(vol, rel=1e-10) and row["area"] == pytest.approx(area, rel=1e-10)
    # the table filtered on the host
    few = _run(capsys, [src, "--threshold", 226, 3071, "--split", tmp_path / "few", "--split-min-triangles",
                        max(len(pf) for _, pf in parts)])
    assert few["split"]["regions"] == 3 and len(few["split"]["parts"]) == 1
    assert len(list((tmp_path / "few").iterdir())) == 1
    # a pick inside the small ball keeps the small ball only
    small = int(np.argmin([len(pf) for _, pf in parts]))
    centre = parts[small][0].astype(np.float64).mean(0)
    stl = tmp_path / "small.stl"
    res = _run(capsys, [src, "--threshold", 226, 3071, "--surface-seed", *centre.tolist(), "--stl", stl])
    assert res["surface_seed"]["point_ids"] == [pu.nearest_point(verts, centre)]
    assert res["surface_seed"]["triangles"] == len(parts[small][1])
    assert np.array_equal(_stl_triangles(stl), parts[small][0][parts[small][1]])
    sv, sf = pu.JoinSeedsParts(verts, faces, res["surface_seed"]["point_ids"])
    assert np.array_equal(sv[sf], parts[small][0][parts[small][1]])
