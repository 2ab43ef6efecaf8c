"""The cases of tests/golden/ref_editor.npz (made by tests/golden/make_golden_ref_editor.py from the reference's own methods),
decoded for the CPU and the GPU tests of the slice editing tools."""
import functools
import os

import numpy as np

ORIENTATIONS = ("AXIAL", "CORONAL", "SAGITAL")
METHODS = ("threshold", "dynamic", "confidence")
# the facts of a 7 x 7 disk on a 20 x 20 slice: position -> (pixels written, first and last column written or None)
DISK_20 = {(3, 3): (29, 0, 6), (2, 2): (29, 0, 6), (1, 5): (28, 0, 5), (0, 0): (18, 0, 4), (-4, 5): (1, 0, 0), (-5, 5): (0, None, None),
           (-8, 5): (0, None, None), (23, 10): (0, None, None), (30, 10): (0, None, None), (10, -9): (0, None, None),
           (22, 10): (1, 19, 19), (5.5, 5.5): (29, 3, 9)}


@functools.lru_cache(maxsize=1)
def golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_editor.npz")
    return dict(np.load(path))


def footprint(k):
    return golden()["footprint_%d" % int(k)]


def position(row):
    """the (px, py, is_flat) triple of a meta row as the reference was given it"""
    px, py, flat = row
    if flat:
        return int(px)
    return tuple(int(v) if float(v).is_integer() else float(v) for v in (px, py))


def dab_cases(vol):
    """(orientation, n, operation, footprint number, position, golden buffer slice) of every recorded dab of 'small' or 'big'"""
    g = golden()
    for ori in ORIENTATIONS:
        meta, outs = g["dabs_%s_%s_meta" % (vol, ori)], g["dabs_%s_%s_out" % (vol, ori)]
        for row, out in zip(meta, outs):
            yield ori, int(row[0]), int(row[1]), int(row[2]), position(row[3:6]), out


def volume(vol):
    g = golden()
    return (g["img"], g["mask_in"]) if vol == "small" else (g["big_img"], g["big_mask_in"])


def slice_of(a, orientation, n):
    return a[n] if orientation == "AXIAL" else (a[:, n, :] if orientation == "CORONAL" else a[:, :, n])
