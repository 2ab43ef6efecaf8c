"""CPU: the host side of the density measures.  invesalius3_amd/math_utils.py, the measures' area and perimeter and
the records' dicts equal the numbers the reference itself produced (tests/golden/ref_density.npz); the selection predicates
the kernels run (csrc/density_roi_math.h, built with the host compiler) equal the numpy restatement (tests/_density_ref.py)
for every pixel; the restatement's ellipse statistics equal the reference's."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import _density_ref as R
from invesalius3_amd import _lib as L
from invesalius3_amd import math_utils as mu
from invesalius3_amd import measures as M

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "ref_density.npz"))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/density_roi_host_emu.cpp: the header the kernels include, built with the host compiler (no FMA contraction)"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("density_emu") / "emu")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "density_roi_host_emu.cpp")],
                   check=True)

    def run(rule, a, b, *args, points=None):
        argv = [exe, rule, str(a), str(b)] + [repr(float(v)) for v in args]
        stdin = b""
        if points is not None:
            pts = np.ascontiguousarray(points, np.float64).reshape(-1, 2)
            argv.append(str(len(pts)))
            stdin = pts.tobytes()
        r = subprocess.run(argv, input=stdin, capture_output=True, check=True)
        return np.frombuffer(r.stdout, np.uint8).reshape(a, b).astype(bool)
    return run


def ellipse_cases(G):
    """(volume, orientation, slice, spacing, center, point1, point2, reference's output row, what it raised)"""
    for row, out, err in zip(G["ellipse_cases"], G["ellipse_out"], G["ellipse_raised"]):
        yield (G["volume_%d" % int(row[0])], R.ORIENTATIONS[int(row[1])], int(row[2]), tuple(row[3:6]), tuple(row[6:9]), tuple(row[9:12]),
               tuple(row[12:15]), out, str(err))


# ---- the reference's own numbers --------------------------------------------------------------------------------------------
def test_constants_equal_the_reference(G):
    assert list(G["constants"]) == [M.AXIAL, M.CORONAL, M.SAGITAL, M.LINEAR, M.ANGULAR, M.DENSITY_ELLIPSE, M.DENSITY_POLYGON, M.SURFACE]
    assert str(G["name_pattern"]) == M.MEASURE_NAME_PATTERN


def test_math_utils_equal_the_reference(G):
    for k, (p, q) in enumerate(G["mu_points"]):
        assert mu.calculate_distance(tuple(p), tuple(q)) == G["mu_distance"][k]
        assert mu.calculate_distance(tuple(p[:2]), tuple(q[:2])) == G["mu_distance_2d"][k]
        assert mu.calculate_angle(tuple(p), tuple(q)) == G["mu_angle"][k]
    for k, (a, b) in enumerate(G["mu_ab"]):
        assert mu.calc_ellipse_area(float(a), float(b)) == G["mu_ellipse_area"][k]
        assert mu.calc_ellipse_circumference(float(a), float(b)) == G["mu_ellipse_circumference"][k]
    for k in range(len(G["mu_poly_area"])):
        pts = [tuple(v) for v in G["mu_poly_%d" % k].tolist()]
        assert mu.calc_polygon_area(pts) == G["mu_poly_area"][k]
        assert mu.calc_polygon_perimeter(pts) == G["mu_poly_perimeter"][k]
    assert mu.calc_ellipse_circumference(4.0, 4.0) == np.pi * 4.0  # the radii are halved first: a circle of radius 4 gives 4 pi


def test_area_and_perimeter_equal_the_reference(G):
    n = 0
    for _, ori, sl, sp, c, p1, p2, out, _ in ellipse_cases(G):
        m = M.CircleDensityMeasure(ori, sl, c, p1, p2)
        assert float(m.calc_area()) == out[4] and float(m.calc_perimeter()) == out[5]
        n += 1
    assert n == len(G["ellipse_cases"]) >= 60
    for k, o in enumerate(G["polygon_orientations"]):
        m = M.PolygonDensityMeasure(R.ORIENTATIONS[int(o)], 0, [tuple(p) for p in G["polygon_%d_points" % k].tolist()])
        assert (m.calc_area(), m.calc_perimeter()) == tuple(G["polygon_%d_out" % k])


def test_records_equal_the_reference(G):
    fresh = json.loads(str(G["record_fresh"]))
    mine = M.DensityMeasurement()
    assert not hasattr(mine, "value") and "value" not in fresh
    assert sorted(vars(mine)) == sorted(fresh)
    for key in ("area", "perimeter", "min", "max", "mean", "std", "location", "type", "slice_number", "points", "visible"):
        assert getattr(mine, key) == fresh[key], key
    for info, want in zip(json.loads(str(G["records_in"])), json.loads(str(G["records_out"]))):
        m = M.DensityMeasurement()
        m.Load(info)
        got = m.get_as_dict()
        assert got == want["dict"] and list(got) == list(want["dict"]) and m.perimeter == want["perimeter"]
        assert "perimeter" not in got and "value" in got
    info = json.loads(str(G["measurement_in"]))
    m = M.Measurement()
    m.Load(info)
    assert m.get_as_dict() == json.loads(str(G["measurement_out"])) and list(m.get_as_dict()) == list(json.loads(str(G["measurement_out"])))
    assert M.Measurement().location == M.SURFACE and M.Measurement().type == M.LINEAR and M.Measurement().value == 0


def test_restatement_statistics_equal_the_reference(G):
    """min, max and mean exactly; std exactly against the rational rule and within the pairwise-summation bound of the reference"""
    worst, raised = 0.0, 0
    for vol, ori, sl, sp, c, p1, p2, out, err in ellipse_cases(G):
        img = R.slice_of(vol, ori, sl)
        h, w = img.shape
        par = R.ellipse_params(ori, sp, c, p1, p2)
        if err:
            assert err == "IndexError" and R.ogrid_shape(h, w, par[0], par[1]) != (h, w)
            m = M.CircleDensityMeasure(ori, sl, c, p1, p2)
            with pytest.raises(IndexError):
                m._describe(M._Grid.of(vol), sp)
            raised += 1
            continue
        assert R.ogrid_shape(h, w, par[0], par[1]) == (h, w)
        rec = R.record(img[R.ellipse_mask(h, w, *par)])
        st = R.stats(rec)
        assert st[:3] == tuple(out[:3]) and out[6] == st[2], (ori, sl, sp, c)
        assert M.stats_from_record(rec) == (st if rec[0] else (0, 0, 0, 0))
        if rec[0]:
            rel = abs(st[3] - out[3]) / out[3] if out[3] else abs(st[3])
            worst = max(worst, rel)
            assert rel <= R.pairwise_bound(rec[0]), (rel, rec[0])
        else:
            assert tuple(out[:4]) == (0.0, 0.0, 0.0, 0.0)
    assert raised == 1
    print("largest relative deviation of std from the reference's float over the fixture: %.3g" % worst)


# ---- the header against the restatement ---------------------------------------------------------------------------------------
def test_header_rule_e_equals_the_restatement_on_the_fixture(G, emu):
    some = 0
    for vol, ori, sl, sp, c, p1, p2, out, err in ellipse_cases(G):
        h, w = R.slice_of(vol, ori, sl).shape
        par = R.ellipse_params(ori, sp, c, p1, p2)
        want = R.ellipse_mask(h, w, *par)
        assert np.array_equal(emu("e", h, w, *par), want), (ori, sl, sp, c)
        some += int(want.any())
    assert some >= 30


def test_rule_e_selects_pixels_on_the_boundary(emu):
    """spacing 0.5 with centre and radii on the half-integer grid: the axis end points satisfy the rule with equality"""
    sx = sy = 0.5
    cx, cy, a, b = 4.5, 3.5, 2.5, 1.5
    got = emu("e", 16, 20, sx, sy, cx, cy, a ** 2, b ** 2)
    assert np.array_equal(got, R.ellipse_mask(16, 20, sx, sy, cx, cy, a ** 2, b ** 2))
    for i, j in ((4, 7), (14, 7), (9, 4), (9, 10)):  # (cx -+ a) / sx, (cy -+ b) / sy
        assert got[j, i]
    assert not got[7, 3] and not got[7, 15] and not got[3, 9] and not got[11, 9]
    assert got.sum() == sum(1 for j in range(16) for i in range(20) if ((i * sx - cx) ** 2) / a ** 2 + ((j * sy - cy) ** 2) / b ** 2 <= 1.0)
    # a == 0: inf or nan, nothing selected -- not even the centre
    assert not emu("e", 8, 8, 1.0, 1.0, 4.0, 4.0, 0.0, 9.0).any() and not emu("e", 8, 8, 1.0, 1.0, 4.0, 4.0, 9.0, 0.0).any()


POLYGONS = {
    "square_through_centres": [(2.5, 2.5), (9.5, 2.5), (9.5, 7.5), (2.5, 7.5)],  # vertices and horizontal edges exactly on pixel centres
    "concave": [(1.0, 1.0), (12.0, 1.5), (12.5, 10.0), (7.0, 4.5), (1.5, 10.5)],
    "self_intersecting": [(1.5, 1.5), (11.5, 9.5), (11.5, 1.5), (1.5, 9.5)],  # a bow tie (odd-even)
    "pentagram": [(8.0, 0.5), (11.0, 11.5), (1.0, 4.5), (15.0, 4.5), (5.0, 11.5)],  # the middle is wound twice: outside by odd-even
    "off_slice": [(-5.0, -4.0), (30.0, -3.0), (8.0, 6.5)],
    "none": [], "one": [(3.0, 3.0)], "two": [(1.0, 1.0), (9.0, 9.0)],
}


def test_header_rule_p_equals_the_restatement(emu):
    h, w = 12, 16
    for name, pts in POLYGONS.items():
        want = R.polygon_mask(h, w, pts)
        assert np.array_equal(emu("p", h, w, points=pts), want), name
        assert want.any() == (len(pts) >= 3), name
    sq = R.polygon_mask(h, w, POLYGONS["square_through_centres"])
    # the crossing test is half-open: the low edges (centres at 2.5) are inside, the high ones (9.5, 7.5) outside
    assert sq[2, 2] and sq[2, 8] and not sq[2, 9] and sq[6, 2] and not sq[7, 2] and sq.sum() == 7 * 5
    star = R.polygon_mask(h, w, POLYGONS["pentagram"])
    assert not star[5, 8] and star[2, 8]  # odd-even: the pentagon in the middle is a hole
    bow = R.polygon_mask(h, w, POLYGONS["self_intersecting"])
    assert bow[5, 2] and bow[5, 10] and not bow[2, 6] and not bow[8, 6]


def test_polygon2mask_predicate_through_the_shared_header(emu):
    """k_polygon2mask now calls polygon_contains of the header: the same mask as the transcription test_oracle_edit.py uses"""
    from test_oracle_edit import _py_polygon

    for shape, pts in (((20, 16), [[2.5, 1.0], [17.2, 3.3], [12.0, 14.9], [6.1, 9.0], [1.0, 12.5]]),
                       ((8, 8), [[-5.0, -5.0], [30.0, -5.0], [30.0, 30.0], [-5.0, 30.0]]),
                       ((12, 9), [[1.0, 1.0], [10.0, 1.0], [10.0, 7.0], [1.0, 7.0]]), ((5, 6), [])):
        want = _py_polygon(shape, pts)
        got = emu("c", shape[0], shape[1], points=pts)
        assert np.array_equal(got, want), shape
        r, c = np.mgrid[:shape[0], :shape[1]]
        assert np.array_equal(R.crossing_mask(r.astype(np.float64), c.astype(np.float64), pts) if len(pts) else np.zeros(shape, bool), want)


# ---- the Python layer without a device -----------------------------------------------------------------------------------------
def test_descriptors_follow_calc_density(G):
    vol = G["volume_0"]
    grid = M._Grid.of(vol)
    for _, ori, sl, sp, c, p1, p2, out, err in ellipse_cases(G):
        if err:
            continue
        q, pts = M.CircleDensityMeasure(ori, sl, c, p1, p2)._describe(grid, sp)
        img = R.slice_of(vol, ori, sl)
        assert (q.h, q.w, q.row_stride, q.elem_stride) == (img.shape + img.strides) and q.image == img.ctypes.data and pts is None
        assert (q.sx, q.sy, q.cx, q.cy, q.a2, q.b2) == R.ellipse_params(ori, sp, c, p1, p2) and q.kind == L.ROI_ELLIPSE
    poly = M.PolygonDensityMeasure("SAGITAL", 3, [(9.0, 1.0, 2.5), (9.0, 4.0, 2.5), (9.0, 2.0, 7.5)])
    q, pts = poly._describe(grid, (0.5, 0.5, 2))
    assert np.array_equal(pts, R.polygon_points("SAGITAL", (0.5, 0.5, 2), poly.points)) and q.n_points == 3 and q.kind == L.ROI_POLYGON
    with pytest.raises(IndexError):
        M.CircleDensityMeasure("AXIAL", 12, (0, 0, 0), (1, 0, 0), (0, 1, 0))._describe(grid, (1, 1, 1))
    with pytest.raises(TypeError):
        M.PolygonDensityMeasure("AXIAL", 0, [(float(k), 0.0, 0.0) for k in range(L.ROI_MAX_POINTS + 1)])._describe(grid, (1, 1, 1))
    with pytest.raises(TypeError):
        M._Grid.of(vol.astype(np.int32))


def test_abi_names_are_declared():
    with open(os.path.join(HERE, "..", "include", "ivx.h")) as f:
        text = f.read()
    lib_text = open(os.path.join(HERE, "..", "invesalius3_amd", "_lib.py")).read()
    for name in ("ivx_dev_roi_density", "ivx_roi_density"):
        assert "int %s(" % name in text and '"%s"' % name in lib_text
    assert "#define IVX_ROI_MAX_POINTS %d" % L.ROI_MAX_POINTS in text and "#define IVX_ROI_RECORD_BYTES %d" % L.ROI_RECORD_BYTES in text
    if os.path.exists(L.LIB_PATH):
        import ctypes
        lib = L.lib()
        assert lib.ivx_roi_density.argtypes and lib.ivx_dev_roi_density.argtypes and ctypes.sizeof(L.Roi) == 152


def test_std_rule_where_floats_cancel():
    rec = R.record(np.full(4000, 32767, np.int16))
    assert M.stats_from_record(rec) == (32767, 32767, 32767.0, 0.0)
    rec = R.record(np.array([-32768, 32767] * 500, np.int16))
    assert M.stats_from_record(rec)[3] == math.sqrt(float(((32767 + 32768) ** 2) / 4.0))
    assert M.stats_from_record((0, 0, 0, 0, 0)) == (0, 0, 0, 0)
