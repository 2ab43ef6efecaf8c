"""Fixtures of the image geometry tools, shared by the CPU and the GPU tests: the slice and the shifts the tilt's
arithmetic is pinned with, the two phantoms, the per-slice shifts of FixGantryTilt and the tool restated over live scipy."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_imagetools.npz")
SHIFTS = (0.0, -0.37, -3.5, -7.25, 2.6, -19.0, -19.01, -25.0)  # the last two fill every row of a 20-row slice
PHANTOM_SPACING = (0.5, 0.5, 1.25)
PHANTOM_TILT = 11.5
TILTS = (0.0, 0.5, 11.5, -20.0, 80.0)  # 80 degrees: from slice 3 on every row of the phantom is filled
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def fixture_slice():
    """20 x 9, random in [-1024, 3000), a flat band of -1024, a block at 32767 and two voxels at -32768: both clamps fire"""
    rng = np.random.default_rng(7)
    s = rng.integers(-1024, 3000, size=(20, 9)).astype(np.int16)
    s[8:11] = -1024
    s[3:6, 2:5] = 32767
    s[14, 6] = s[15, 1] = -32768
    return s


def small_slice(h, w=5, seed=3):
    return np.random.default_rng(seed + h).integers(-1024, 3000, size=(h, w)).astype(np.int16)


def disc_phantom(shape=(12, 40, 16), seed=11):
    """a bright disc of 1500 +- 20 in -1024 air: the spline undershoots next to its edge, so the fill value keeps falling"""
    d, h, w = shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w]
    disc = ((y - h / 2.0) / (h * 0.3)) ** 2 + ((x - w / 2.0) / (w * 0.35)) ** 2 <= 1.0
    vol = np.full(shape, -1024, np.int16)
    vol[:, disc] = (1500 + rng.integers(-20, 21, size=(d, int(disc.sum())))).astype(np.int16)
    return vol


def slice0_min_phantom(shape=(6, 33, 65), seed=12):
    """the global minimum lies in slice 0 alone, which the tool never shifts: every fill value is that voxel's"""
    vol = np.random.default_rng(seed).integers(-500, 2000, size=shape).astype(np.int16)
    vol[0, 5, 7] = -2000
    return vol


def tilt_shifts(depth, spacing, tilt):
    """the first component of the shift FixGantryTilt hands scipy for slice n (imagedata_utils.py:148-154), as it forms it"""
    gntan = math.tan(np.radians(tilt))
    out = np.empty(depth, np.float64)
    for n in range(depth):
        offset = gntan * n * spacing[2]
        out[n] = -offset / spacing[1]
    return out


def scipy_fix_gantry_tilt(matrix, spacing, tilt):
    """the tool over live scipy, in place; returns the fill value every slice was given"""
    from scipy.ndimage import shift

    cvals = []
    for n, s in enumerate(tilt_shifts(matrix.shape[0], spacing, tilt)):
        cvals.append(int(matrix.min()))
        matrix[n] = shift(matrix[n], (s, 0), cval=cvals[-1])
    return cvals
