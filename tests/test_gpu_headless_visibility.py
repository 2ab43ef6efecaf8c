"""Headless driver with the surface visibility tool: .inv3 -> --threshold --largest --remove-nonvisible --stl.  The STL must hold
exactly the triangles of the same chain made by hand with the Python calls: a hollow ball whose cavity opens to the outside
through a narrow tunnel (ONE connected surface, most of it hidden) next to a small ball goes in; the outside of the hollow ball
and what the tunnel shows of its inside come out."""
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
    z, y, x = np.mgrid[:26, :26, :40]
    d2 = (z - 12.5) ** 2 + (y - 12.5) ** 2 + (x - 12.5) ** 2
    img = np.full(z.shape, -1000, np.int16)
    img[(d2 <= 10.0 ** 2) & (d2 > 5.0 ** 2)] = 1000                                # a ball with a cavity ...
    img[(abs(z - 12.5) < 1) & (abs(y - 12.5) < 1) & (x <= 12)] = -1000             # ... that a 2 x 2 tunnel joins to the outside
    img[(z - 12.5) ** 2 + (y - 12.5) ** 2 + (x - 32.5) ** 2 <= 4.0 ** 2] = 1200  # ... and a small one apart from it
    return img


def _stl_triangles(path):
    raw = open(path, "rb").read()
    n = struct.unpack("<I", raw[80:84])[0]
    rec = np.frombuffer(raw[84:], dtype=[("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")])
    assert n == len(rec)
    return rec["v"]


def test_threshold_largest_remove_nonvisible_stl(ivxlib, tmp_path, capsys):
    from invesalius3_amd import polydata_utils as pu
    from invesalius3_amd import project as prj
    from invesalius3_amd import surface_process as sp
    img = _image()
    p = prj.Project(name="Shells", spacing=SPACING, threshold_range=(int(img.min()), int(img.max())))
    p.matrix = img
    src = tmp_path / "in.inv3"
    prj.save_inv3(src, p)
    stl, stl_all = tmp_path / "shell.stl", tmp_path / "all.stl"
    res = _run(capsys, [src, "--threshold", 226, 3071, "--largest", "--remove-nonvisible", "--stl", stl])
    # the chain by hand
    mask = np.where((img >= 226) & (img <= 3071), 255, 0).astype(np.uint8)
    verts, faces = sp.marching_cubes_indexed(mask, SPACING, [127.0], 0, True, True, True, 0.0, 1)
    assert res["surface"] == {"vertices": len(verts), "triangles": len(faces)}
    v1, f1, nreg = sp.keep_largest(verts, faces)
    assert nreg == 2 and res["largest"] == {"regions": 2, "vertices": len(v1), "triangles": len(f1)}
    v2, f2 = pu.RemoveNonVisibleFaces(v1, f1)
    assert 0 < len(f2) < len(f1)
    assert res["remove_nonvisible"] == {"vertices": len(v2), "triangles": len(f2), "removed_triangles": len(f1) - len(f2)}
    assert np.array_equal(_stl_triangles(stl), v2[f2])
    vol, area = sp.mass_properties(v2, f2)
    assert res["volume"] == pytest.approx(vol, rel=1e-10) and res["area"] == pytest.approx(area, rel=1e-10)
    # without the option the cavity's wall stays in the file; and the option alone leaves both balls' outsides
    res = _run(capsys, [src, "--threshold", 226, 3071, "--largest", "--stl", stl_all])
    assert "remove_nonvisible" not in res and np.array_equal(_stl_triangles(stl_all), v1[f1])
    res = _run(capsys, [src, "--threshold", 226, 3071, "--remove-nonvisible", "--stl", stl_all])
    v3, f3 = pu.RemoveNonVisibleFaces(verts, faces)
    assert np.array_equal(_stl_triangles(stl_all), v3[f3]) and len(f2) < len(f3) < len(faces)
