"""numpy restatement of the density measures: rule E (the reference's ellipse, measures.py:2062-2064), rule P (the
project's statement of the wx polygon fill), the statistics and the orientation picks of calc_density.  Independent of the
product: the tests hold the header (csrc/density_roi_math.h), the kernel and invesalius3_amd/measures.py to it."""
import math
from fractions import Fraction

import numpy as np

ORIENTATIONS = {1: "AXIAL", 2: "CORONAL", 3: "SAGITAL"}
PLANE = {"AXIAL": (0, 1), "CORONAL": (0, 2), "SAGITAL": (1, 2)}  # the in-plane coordinates of (x, y, z): columns, rows


def slice_of(volume, orientation, n):
    if orientation == "AXIAL":
        return volume[n]
    return volume[:, n, :] if orientation == "CORONAL" else volume[:, :, n]


def ellipse_params(orientation, spacing, center, point1, point2):
    """sx, sy, cx, cy, a2, b2 as calc_density picks them; the squares are Python's ``**``"""
    i, j = PLANE[orientation]
    a, b = abs(point1[i] - center[i]), abs(point2[j] - center[j])
    return float(spacing[i]), float(spacing[j]), float(center[i]), float(center[j]), float(a ** 2), float(b ** 2)


def ogrid_shape(h, w, sx, sy):
    gy, gx = np.ogrid[0:h * sy:sy, 0:w * sx:sx]
    return gy.shape[0], gx.shape[1]


def ellipse_mask(h, w, sx, sy, cx, cy, a2, b2):
    """rule E: pixel (j, i) stands at (i * sx, j * sy)"""
    x = np.arange(w, dtype=np.float64) * np.float64(sx)
    y = np.arange(h, dtype=np.float64) * np.float64(sy)
    with np.errstate(all="ignore"):
        tx = ((x - cx) * (x - cx)) / np.float64(a2)
        ty = ((y - cy) * (y - cy)) / np.float64(b2)
        return (tx[None, :] + ty[:, None]) <= 1.0


def crossing_mask(px, py, pts):
    """odd-even rule: the crossing test of polygon2mask_rs for the sample points (px, py), arrays of one shape"""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    inside = np.zeros(np.broadcast(px, py).shape, bool)
    n = len(pts)
    with np.errstate(all="ignore"):
        for k in range(n):
            xi, yi = pts[k]
            xj, yj = pts[k - 1]
            inside ^= ((yi > py) != (yj > py)) & (px < (xj - xi) * (py - yi) / (yj - yi) + xi)
    return inside


def polygon_mask(h, w, pts):
    """rule P: pixel (j, i) is its centre (i + 0.5, j + 0.5); fewer than three points select nothing"""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    if len(pts) < 3:
        return np.zeros((h, w), bool)
    return crossing_mask((np.arange(w, dtype=np.float64) + 0.5)[None, :], (np.arange(h, dtype=np.float64) + 0.5)[:, None], pts)


def polygon_points(orientation, spacing, points):
    i, j = PLANE[orientation]
    return np.array([(p[i] / spacing[i], p[j] / spacing[j]) for p in points], np.float64).reshape(-1, 2)


def record(values):
    """cnt, s1, s2, lo, hi as exact integers (zeros for an empty selection)"""
    v = [int(x) for x in np.asarray(values).ravel()]
    if not v:
        return (0, 0, 0, 0, 0)
    return (len(v), sum(v), sum(x * x for x in v), min(v), max(v))


def stats(rec):
    """min, max, mean, std by the exact-rational rule"""
    cnt, s1, s2, lo, hi = rec
    if cnt == 0:
        return (0.0, 0.0, 0.0, 0.0)
    return (float(lo), float(hi), float(s1) / float(cnt), math.sqrt(float(Fraction(cnt * s2 - s1 * s1, cnt * cnt))))


def pairwise_bound(cnt):
    """relative bound on the difference between numpy's ``values.std()`` (pairwise float64 summation) and the exact value"""
    return (math.log2(max(cnt, 1)) + 8) * 2.0 ** -52
