"""Golden numbers from the REFERENCE ITSELF for the density measures: what its own Python computes without a
canvas.  The reference's modules are imported from its checkout (INVESALIUS_REFERENCE) under the stand-in finder and the
methods called unbound on plain namespaces.

    INVESALIUS_REFERENCE=<the reference's checkout> python3 tests/golden/make_golden_ref_density.py

Recorded: CircleDensityMeasure.calc_density (min, max, mean, std, area, perimeter, value as it stores them on its measurement,
or the exception's name), calc_area and calc_perimeter; PolygonDensityMeasure.calc_area and calc_perimeter;
DensityMeasurement.Load / get_as_dict; the six functions of invesalius/math_utils.py.  PolygonDensityMeasure.calc_density
needs a live wx canvas and is not here.  Arrays, names and JSON text of dicts only.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ref_dowatershed as M  # noqa: E402

ORI = {"AXIAL": 1, "CORONAL": 2, "SAGITAL": 3}
SPACINGS = [(1, 1, 1), (0.5, 0.5, 2), (0.488281, 0.488281, 1.25)]
SHAPE = (12, 14, 16)  # dz, dy, dx


def volume():
    rng = np.random.default_rng(20)
    v = rng.integers(-60, 60, SHAPE).astype(np.int16)
    z, y, x = np.meshgrid(*[np.arange(s) for s in SHAPE], indexing="ij")
    v += (40 * (z + y) - 25 * x).astype(np.int16)
    v[3, 4, 5], v[6, 7, 8], v[5, 6, 7] = -32768, 32767, 32767
    return v


def ellipse_cases():
    """(volume index, orientation, slice, spacing, center, point1, point2)"""
    cases = []
    for sp in SPACINGS:
        ext = [SHAPE[2] * sp[0], SHAPE[1] * sp[1], SHAPE[0] * sp[2]]  # x, y, z in mm
        mid = [e / 2 for e in ext]
        for name, n in (("AXIAL", 5), ("CORONAL", 6), ("SAGITAL", 7)):
            i, j = {"AXIAL": (0, 1), "CORONAL": (0, 2), "SAGITAL": (1, 2)}[name]

            def at(ci, cj, ra, rb):
                c, p1, p2 = list(mid), list(mid), list(mid)
                c[i], c[j] = ci, cj
                p1[i], p1[j] = ci + ra, cj
                p2[i], p2[j] = ci, cj - rb
                return tuple(c), tuple(p1), tuple(p2)

            q = [sp[i], sp[j]]
            cases.append((0, name, n, sp) + at(6 * q[0], 5 * q[1], 3 * q[0], 2 * q[1]))           # inside, on the pixel grid: equality
            cases.append((0, name, n, sp) + at(6.3 * q[0], 5.2 * q[1], 3.7 * q[0], 2.9 * q[1]))   # inside, off the grid
            cases.append((0, name, n, sp) + at(0.5 * q[0], ext[j] - q[1], 4 * q[0], 3.5 * q[1]))  # cut by two edges
            cases.append((0, name, n, sp) + at(-9 * q[0], 3 * q[1], 3 * q[0], 2 * q[1]))          # wholly outside
            cases.append((0, name, n, sp) + at(ext[i] * 3, ext[j] * 3, 2 * q[0], 2 * q[1]))       # far outside
            cases.append((0, name, n, sp) + at(mid[i], mid[j], 100 * q[0], 100 * q[1]))           # covers the slice
        c = (4 * sp[0], 4 * sp[1], 0.0)
        cases.append((0, "AXIAL", 2, sp, c, c, (c[0], c[1] + 3 * sp[1], 0.0)))  # a == 0
        cases.append((0, "AXIAL", 2, sp, c, (c[0] + 2 * sp[0], c[1], 0.0), c))  # b == 0
    # np.ogrid's length quirk: 3 pixels at spacing 0.1 give an axis of 4
    cases.append((1, "AXIAL", 1, (0.1, 1.0, 1.0), (0.1, 2.0, 0.0), (0.2, 2.0, 0.0), (0.1, 3.0, 0.0)))
    return cases


POLYGONS = [
    ("AXIAL", [(1.0, 1.0, 3.0), (9.5, 2.0, 3.0), (7.25, 8.0, 3.0), (2.0, 6.5, 3.0)]),
    ("CORONAL", [(0.0, 4.0, 0.0), (6.0, 4.0, 0.0), (6.0, 4.0, 5.0), (3.0, 4.0, 2.0), (0.0, 4.0, 5.0)]),
    ("SAGITAL", [(2.0, 1.5, 1.5), (2.0, 7.5, 7.5), (2.0, 7.5, 1.5), (2.0, 1.5, 7.5)]),
    ("AXIAL", [(0.3, 0.1, 0.0), (4.7, 0.9, 0.0), (2.2, 3.3, 0.0)]),
    ("AXIAL", [(1.0, 1.0, 0.0), (2.0, 2.0, 0.0)]),
]

RECORDS = [
    {"index": 3, "name": "M 4", "colour": [1, 0.4, 0], "value": 12.5, "location": 1, "type": 8, "slice_number": 7,
     "points": [[1.0, 2.0, 3.0], [4.0, 2.0, 3.0], [1.0, 6.0, 3.0]], "visible": True, "area": 37.7, "min": -5.0, "max": 90.0,
     "mean": 12.5, "std": 3.25, "perimeter": 11.05},
    {"index": 0, "name": "poly", "colour": [0, 0, 1], "value": 1.0, "location": 3, "type": 9, "slice_number": 0,
     "points": [[0.0, 1.0, 1.0], [0.0, 5.0, 1.0], [0.0, 3.0, 3.0]], "visible": False, "area": 4.0, "min": 0.0, "max": 2.0,
     "mean": 1.0, "std": 0.5},
]


def main(path):
    tmp_root = tempfile.mkdtemp(prefix="ref_density_")
    tempfile.tempdir = tmp_root
    os.environ["HOME"] = tmp_root
    sys.meta_path.insert(0, M._Finder())
    import pubsub.pub
    pubsub.pub.subscribe = lambda *a, **k: (None, True)
    pubsub.pub.sendMessage = lambda *a, **k: None
    reference = os.environ.get("INVESALIUS_REFERENCE")
    if not reference or not os.path.isdir(os.path.join(reference, "invesalius")):
        raise SystemExit("set INVESALIUS_REFERENCE to the reference's checkout (the directory that holds invesalius/)")
    sys.path.insert(0, reference)
    from invesalius import constants as const
    from invesalius import math_utils as mu
    from invesalius.data import slice_ as rs  # (first: the reference's import cycle resolves from this end)
    from invesalius.data import measures as rm

    d = {}
    d["constants"] = np.array([const.AXIAL, const.CORONAL, const.SAGITAL, const.LINEAR, const.ANGULAR, const.DENSITY_ELLIPSE,
                               const.DENSITY_POLYGON, const.SURFACE], np.int64)
    d["name_pattern"] = np.array(str(const.MEASURE_NAME_PATTERN))
    vols = [volume(), (np.arange(4 * 5 * 3, dtype=np.int16) * 7 - 100).reshape(4, 5, 3)]
    d["volume_0"], d["volume_1"] = vols

    # CircleDensityMeasure.calc_density: the Slice singleton it asks for is a namespace around the volume
    state = {}

    def fake_slice():
        v, sp = vols[state["vol"]], state["spacing"]

        def get_image_slice(orientation, n, *a, **k):
            return {"AXIAL": v[n], "CORONAL": v[:, n, :], "SAGITAL": v[:, :, n]}[orientation]

        mask = np.zeros(tuple(s + 1 for s in v.shape), np.uint8)
        return types.SimpleNamespace(get_image_slice=get_image_slice, spacing=sp, current_mask=types.SimpleNamespace(matrix=mask),
                                     buffer_slices={o: types.SimpleNamespace(index=0) for o in ORI})

    rs.Slice = fake_slice
    rows, outs, raised = [], [], []
    for vol, name, n, sp, c, p1, p2 in ellipse_cases():
        state["vol"], state["spacing"] = vol, sp
        meas = types.SimpleNamespace()
        me = types.SimpleNamespace(slice_number=n, orientation=name, center=c, point1=p1, point2=p2, _measurement=meas,
                                   set_density_values=lambda *a: None)
        me.calc_area = lambda me=me: rm.CircleDensityMeasure.calc_area(me)
        me.calc_perimeter = lambda me=me: rm.CircleDensityMeasure.calc_perimeter(me)
        err = ""
        try:
            with np.errstate(all="ignore"):
                rm.CircleDensityMeasure.calc_density(me)
            out = [meas.min, meas.max, meas.mean, meas.std, meas.area, meas.perimeter, meas.value]
            assert meas.points == [c, p1, p2] and all(type(v) is float for v in out)
        except IndexError as e:
            err, out = type(e).__name__, [0.0] * 7
            out[4], out[5] = float(me.calc_area()), float(me.calc_perimeter())
        rows.append([vol, ORI[name], n, *sp, *c, *p1, *p2])
        outs.append(out)
        raised.append(err)
        print(name, n, sp, "->", err or out)
    d["ellipse_cases"] = np.array(rows, np.float64)
    d["ellipse_out"] = np.array(outs, np.float64)
    d["ellipse_raised"] = np.array(raised)

    # PolygonDensityMeasure.calc_area / calc_perimeter (they print what they compute)
    d["polygon_orientations"] = np.array([ORI[o] for o, _ in POLYGONS], np.int64)
    for k, (o, pts) in enumerate(POLYGONS):
        me = types.SimpleNamespace(orientation=o, points=pts)
        d["polygon_%d_points" % k] = np.array(pts, np.float64)
        d["polygon_%d_out" % k] = np.array([rm.PolygonDensityMeasure.calc_area(me), rm.PolygonDensityMeasure.calc_perimeter(me)], np.float64)

    # DensityMeasurement: a fresh record's attributes, Load and get_as_dict
    fresh = rm.DensityMeasurement()
    d["record_fresh"] = np.array(json.dumps({k: v for k, v in sorted(vars(fresh).items())}))
    loaded = []
    for info in RECORDS:
        m = rm.DensityMeasurement()
        m.Load(info)
        loaded.append({"dict": m.get_as_dict(), "perimeter": m.perimeter})
    d["records_in"] = np.array(json.dumps(RECORDS))
    d["records_out"] = np.array(json.dumps(loaded))
    fresh = rm.Measurement()
    info = {"index": 5, "name": "line", "colour": [1, 0, 0], "value": 3.5, "location": 5, "type": 6, "slice_number": 0,
            "points": [[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]], "visible": True}
    fresh.Load(info)
    d["measurement_in"], d["measurement_out"] = np.array(json.dumps(info)), np.array(json.dumps(fresh.get_as_dict()))

    # math_utils
    rng = np.random.default_rng(21)
    pairs = rng.uniform(-50, 50, (8, 2, 3))
    d["mu_points"] = pairs
    d["mu_distance"] = np.array([mu.calculate_distance(tuple(p), tuple(q)) for p, q in pairs], np.float64)
    d["mu_distance_2d"] = np.array([mu.calculate_distance(tuple(p[:2]), tuple(q[:2])) for p, q in pairs], np.float64)
    d["mu_angle"] = np.array([mu.calculate_angle(tuple(p), tuple(q)) for p, q in pairs], np.float64)
    ab = np.concatenate([rng.uniform(0, 80, (8, 2)), [[0.0, 0.0], [0.0, 3.5], [1e-3, 1e3]]])
    d["mu_ab"] = ab
    d["mu_ellipse_area"] = np.array([mu.calc_ellipse_area(float(a), float(b)) for a, b in ab], np.float64)
    d["mu_ellipse_circumference"] = np.array([mu.calc_ellipse_circumference(float(a), float(b)) for a, b in ab], np.float64)
    polys = [rng.uniform(-20, 20, (n, 2)) for n in (3, 4, 7, 12)] + [np.array([[0.0, 0.0], [0.0, 2.0], [2.0, 2.0], [2.0, 0.0]])]
    for k, p in enumerate(polys):
        d["mu_poly_%d" % k] = p
    d["mu_poly_area"] = np.array([mu.calc_polygon_area([tuple(v) for v in p.tolist()]) for p in polys], np.float64)
    d["mu_poly_perimeter"] = np.array([mu.calc_polygon_perimeter([tuple(v) for v in p.tolist()]) for p in polys], np.float64)
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path), "bytes,", len(d), "arrays")


if __name__ == "__main__":
    main(os.path.join(HERE, "ref_density.npz"))
