#!/usr/bin/env python3
"""The density measures on a bound (resident) image against what the package offered before them, in one run:

  bound      measures.density_of on the bound image: descriptors (and a polygon's points) up, one memset and one launch that
             reads the slice's box in the mirror, 40 bytes per measure down
  parent     slice_.get_image_slice on the same bound array (the slice gathered from the mirror and downloaded), then the numpy
             restatement of rules E / P and of the statistics (tests/_density_ref.py) on the host -- the only route without
             the feature
  resident   DeviceVolume.roi_density on a resident volume

Cases: one ellipse of radius 20 px and one of radius 200 px per orientation, a 12-point polygon, and a batch of 64 measures (the
parent repeats its route per measure).  Wall clock around the Python calls (they end synchronised), median of five after a
warm-up, min / max and the bytes the library's copy helpers moved per call beside it.

    python tools/bench_density.py               # 512^3 image -> profiles/bench_density_512.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

p = argparse.ArgumentParser()
p.add_argument("--size", type=int, default=512)
p.add_argument("--reps", type=int, default=5)
p.add_argument("--out", default=None)
args = p.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _density_ref as R  # noqa: E402
from bench import synth_v512  # noqa: E402
from invesalius3_amd import _lib as L  # noqa: E402
from invesalius3_amd import measures as M  # noqa: E402
from invesalius3_amd import resident, slice_  # noqa: E402
from invesalius3_amd.device import DeviceVolume  # noqa: E402

ORIENTATIONS = ("AXIAL", "CORONAL", "SAGITAL")
SPACING = (0.5, 0.5, 0.5)


def timeit(fn):
    t, moved = [], None
    for i in range(args.reps + 1):
        c0 = resident.transfer_stats()
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i:
            t.append(dt)
            moved = {k: v - c0[k] for k, v in resident.transfer_stats().items()}
    return {"ms": round(float(np.median(t)) * 1e3, 3), "min_ms": round(min(t) * 1e3, 3), "max_ms": round(max(t) * 1e3, 3), "calls": len(t),
            "moved_per_call": moved}


def ellipse(ori, n, radius_px):
    i, j = R.PLANE[ori]
    c = [n * SPACING[0] / 2 + 0.1] * 3
    p1, p2 = list(c), list(c)
    p1[i] += radius_px * SPACING[i]
    p2[j] += radius_px * SPACING[j]
    return M.CircleDensityMeasure(ori, n // 2, tuple(c), tuple(p1), tuple(p2))


def polygon(ori, n, npts=12, radius_px=60.0):
    i, j = R.PLANE[ori]
    pts = []
    for k in range(npts):
        a = 2 * np.pi * k / npts
        r = radius_px * (1.0 if k % 2 else 0.55)
        q = [n * SPACING[0] / 2] * 3
        q[i] += r * np.cos(a) * SPACING[i]
        q[j] += r * np.sin(a) * SPACING[j]
        pts.append(tuple(q))
    return M.PolygonDensityMeasure(ori, n // 2, pts)


def restated(img, m):
    """the parent's route for one measure: the slice to the host, rule E / P and the statistics in numpy"""
    sl = slice_.get_image_slice(img, m.orientation, m.slice_number)
    h, w = sl.shape
    if isinstance(m, M.CircleDensityMeasure):
        mask = R.ellipse_mask(h, w, *R.ellipse_params(m.orientation, SPACING, m.center, m.point1, m.point2))
    else:
        mask = R.polygon_mask(h, w, R.polygon_points(m.orientation, SPACING, m.points))
    v = sl[mask]
    return (float(v.min()), float(v.max()), float(v.mean()), float(v.std())) if v.size else (0.0, 0.0, 0.0, 0.0)


def main():
    n = args.size
    L.require_device()
    img = synth_v512((n, n, n))
    res = {}
    t0 = time.perf_counter()
    bound = slice_.bind_image(img)
    res["bind_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    cases = {}
    for ori in ORIENTATIONS:
        cases["ellipse r=20 px, %s" % ori] = [ellipse(ori, n, 20)]
        cases["ellipse r=200 px, %s" % ori] = [ellipse(ori, n, min(200, n // 2 - 2))]
    cases["polygon of 12 points, AXIAL"] = [polygon("AXIAL", n)]
    rng = np.random.default_rng(5)
    batch = []
    for k in range(64):
        ori = ORIENTATIONS[k % 3]
        m = ellipse(ori, n, int(rng.integers(8, 60))) if k % 4 else polygon(ori, n, 12, float(rng.integers(20, 80)))
        m.slice_number = int(rng.integers(0, n))
        batch.append(m)
    cases["batch of 64 measures"] = batch
    for name, ms in cases.items():
        e = res.setdefault(name, {})
        got = M.density_of(img, SPACING, ms)
        want = [restated(img, m) for m in ms]
        for g, w in zip(got, want):  # the same numbers (std: the host's float against the exact rule)
            assert (g["min"], g["max"], g["mean"]) == w[:3] and abs(g["std"] - w[3]) <= 1e-12 * max(w[3], 1.0), (name, g, w)
        e["pixels selected"] = int(sum(R.record(slice_.get_image_slice(img, m.orientation, m.slice_number)[
            R.ellipse_mask(n, n, *R.ellipse_params(m.orientation, SPACING, m.center, m.point1, m.point2)) if isinstance(m, M.CircleDensityMeasure)
            else R.polygon_mask(n, n, R.polygon_points(m.orientation, SPACING, m.points))])[0] for m in ms))
        e["bound"] = timeit(lambda: M.density_of(img, SPACING, ms))
        e["parent"] = timeit(lambda: [restated(img, m) for m in ms])
        e["parent, get_image_slice alone"] = timeit(lambda: [slice_.get_image_slice(img, m.orientation, m.slice_number) for m in ms])
        e["bound / parent"] = round(e["bound"]["ms"] / e["parent"]["ms"], 3)
        e["bound / parent's get_image_slice"] = round(e["bound"]["ms"] / e["parent, get_image_slice alone"]["ms"], 3)
    bound.release()
    with DeviceVolume(img, spacing=SPACING) as vol:
        for name, ms in cases.items():
            res[name]["resident"] = timeit(lambda: vol.roi_density(ms))
    out = {"size": "%d^3 image" % n, "device": L.device_name(),
           "protocol": "wall clock around the Python calls, median of %d after one warm-up (min / max beside it); moved_per_call: bytes "
                       "the library's copy helpers moved; parent = slice_.get_image_slice on the same bound array plus the numpy "
                       "restatement of rules E / P and the statistics on the host, once per measure" % args.reps,
           "results": res}
    text = json.dumps(out, indent=1)
    print(text)
    path = args.out or os.path.join(ROOT, "profiles", "bench_density_%d.json" % n)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
