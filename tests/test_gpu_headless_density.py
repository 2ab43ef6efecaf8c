"""Headless driver with the density measures: .inv3 -> --density-ellipse / --density-polygon give what `measures.density_of`
gives on the project's image, --save writes the new entries so that open_inv3 reads them back, and --remeasure rewrites a
stale entry."""
import json

import numpy as np
import pytest

from invesalius3_amd.measures import density_of  # noqa: F401  (the feature under test: without it this file fails at import)

pytestmark = pytest.mark.gpu

SPACING = (0.5, 0.5, 2.0)
ELLIPSE = ("CORONAL", 7, (5.0, 3.5, 12.0), (8.0, 3.5, 12.0), (5.0, 3.5, 20.0))
POLYGON = ("AXIAL", 4, [(1.0, 1.0, 8.0), (9.5, 2.0, 8.0), (7.25, 8.0, 8.0), (2.0, 6.5, 8.0)])


def _run(capsys, argv):
    from invesalius3_amd import headless
    assert headless.main([str(a) for a in argv]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def _project(tmp_path, measurements=None):
    from invesalius3_amd import project as prj
    rng = np.random.default_rng(3)
    img = rng.integers(-1000, 2000, (14, 18, 22)).astype(np.int16)
    p = prj.Project(name="Density", spacing=SPACING, threshold_range=(int(img.min()), int(img.max())))
    p.matrix = img
    if measurements:
        p.measurements = measurements
    src = tmp_path / "in.inv3"
    prj.save_inv3(src, p)
    return src, img


def _flags():
    o, n, c, p1, p2 = ELLIPSE
    po, pn, pts = POLYGON
    return ["--density-ellipse", o, n, *c, *p1, *p2, "--density-polygon", po, pn, *[v for p in pts for v in p]]


def test_flags_json_and_save_round_trip(ivxlib, tmp_path, capsys):
    from invesalius3_amd import measures as M
    from invesalius3_amd import project as prj
    src, img = _project(tmp_path)
    want = M.density_of(img, SPACING, [M.CircleDensityMeasure(*ELLIPSE), M.PolygonDensityMeasure(*POLYGON)])
    assert want[0]["mean"] != 0.0 and want[1]["mean"] != 0.0
    saved, mj = tmp_path / "out.inv3", tmp_path / "m.json"
    res = _run(capsys, [src, *_flags(), "--measures-json", mj, "--save", saved])
    got = res["density"]["measures"]
    assert len(got) == 2 and "surface" not in res and res["saved"] == str(saved)
    for g, w, kind, ori in zip(got, want, (M.DENSITY_ELLIPSE, M.DENSITY_POLYGON), ("CORONAL", "AXIAL")):
        assert {k: g[k] for k in w} == w and g["type"] == kind and g["orientation"] == ori
    with open(mj) as f:
        filed = json.load(f)
    assert filed["measures"] == got and sorted(filed["measurements"]) == ["0", "1"]
    back = prj.open_inv3(saved)
    try:
        assert sorted(back.measurements) == ["0", "1"]
        e, p = back.measurements["0"], back.measurements["1"]
        assert "perimeter" not in e and (e["index"], e["type"], e["location"], e["slice_number"]) == (0, M.DENSITY_ELLIPSE, M.CORONAL, 7)
        assert (p["index"], p["type"], p["location"], p["slice_number"], p["name"]) == (1, M.DENSITY_POLYGON, M.AXIAL, 4, "M 2")
        for entry, w in ((e, want[0]), (p, want[1])):
            assert {k: entry[k] for k in ("min", "max", "mean", "std", "area", "value")} == {k: w[k] for k in ("min", "max", "mean", "std", "area", "value")}
        assert [list(q) for q in e["points"]] == [list(q) for q in ELLIPSE[2:]] and [list(q) for q in p["points"]] == [list(q) for q in POLYGON[2]]
        assert M.density_of(img, SPACING, [e, p]) == want  # the entries describe the same measures
    finally:
        back.close()


def test_remeasure_rewrites_a_stale_entry(ivxlib, tmp_path, capsys):
    from invesalius3_amd import measures as M
    from invesalius3_amd import project as prj
    stale = {"index": 0, "name": "M 1", "colour": [1, 0, 0], "value": -7.0, "location": M.CORONAL, "type": M.DENSITY_ELLIPSE, "slice_number": 7,
             "points": [list(q) for q in ELLIPSE[2:]], "visible": True, "area": 1.0, "min": -7.0, "max": -7.0, "mean": -7.0, "std": -7.0}
    line = {"index": 1, "name": "M 2", "colour": [1, 0.4, 0], "value": 3.5, "location": 5, "type": M.LINEAR, "slice_number": 0,
            "points": [[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]], "visible": True}
    src, img = _project(tmp_path, {"0": stale, "1": line})
    want = M.density_of(img, SPACING, [M.CircleDensityMeasure(*ELLIPSE)])[0]
    saved = tmp_path / "out.inv3"
    res = _run(capsys, [src, "--remeasure", "--save", saved])
    assert res["density"]["remeasured"] == 1 and res["density"]["measures"] == []
    back = prj.open_inv3(saved)
    try:
        e = back.measurements["0"]
        assert {k: e[k] for k in ("min", "max", "mean", "std", "area", "value")} == {k: want[k] for k in ("min", "max", "mean", "std", "area", "value")}
        assert e["name"] == "M 1" and back.measurements["1"] == line
    finally:
        back.close()


def test_density_arguments(tmp_path):
    from invesalius3_amd import headless
    for bad in (["--density-ellipse", "AXIAL", "1", "2"], ["--density-ellipse", "UP", "1", *["0"] * 9], ["--density-polygon", "AXIAL", "1", "2", "3"],
                ["--measures-json", "m.json"]):
        with pytest.raises(SystemExit):
            headless.main([str(tmp_path / "none.inv3"), *bad])
