#!/usr/bin/env python3
"""The brush of the manual edition panel on bound (resident) matrices, three ways in one run:

  stroke kernel, bound    slice_.edit_mask_stroke on the bound mask and image: the slice is staged from the mirror, one launch
                          per run of one operation, the slice written back to host and mirror
  stroke kernel, unbound  the same call on arrays that are not bound
  numpy + touch           the only route without the feature: the dabs restated in numpy on the host matrix (the reference's own
                          edit_mask_pixel arithmetic), the slice written into the matrix, `Resident.touch(view)` -- which uploads
                          everything between the view's first and last byte again -- and the next use

Every variant is followed by the same next use (a MaxIP of the edited slice's one-slice slab) inside the timed window, so that
the upload a touch only schedules is paid where it belongs.  Per orientation: a 200-dab stroke and a single dab, with a circle
of radius 15 px and of 100 px (BRUSH_MAX_SIZE), BRUSH_THRESH.  Wall clock around the Python calls (they end synchronised), median
of five after a warm-up, min / max and the bytes the library's copy helpers moved per call beside it.

    python tools/bench_editor.py                      # 512^3 image, 513^3 mask
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
p.add_argument("--dabs", type=int, default=200)
args = p.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import BONE, synth_v512  # noqa: E402
from invesalius3_amd import _lib as L  # noqa: E402
from invesalius3_amd import cursor, resident, slice_  # noqa: E402
from invesalius3_amd import mask as mask_mod  # noqa: E402

ORIENTATIONS = ("AXIAL", "CORONAL", "SAGITAL")
EDITION = (226, 3071)


def slice_view(a, orientation, n):
    return a[n] if orientation == "AXIAL" else (a[:, n, :] if orientation == "CORONAL" else a[:, :, n])


def slab(a, orientation, n):
    return a[n:n + 1] if orientation == "AXIAL" else (a[:, n:n + 1, :] if orientation == "CORONAL" else a[:, :, n:n + 1])


def numpy_dab(mask, image, index, position, thresh):
    """Slice.edit_mask_pixel, BRUSH_THRESH (invesalius/data/slice_.py:690-727), on the 2-D buffer slice"""
    px, py = position
    xi = int(px - index.shape[1] + (index.shape[1] / 2 + 1))
    yi = int(py - index.shape[0] + (index.shape[0] / 2 + 1))
    xf, yf = xi + index.shape[1], yi + index.shape[0]
    if yi < 0:
        index, yi = index[abs(yi):, :], 0
    if yf > image.shape[0]:
        index, yf = index[: index.shape[0] - (yf - image.shape[0]), :], image.shape[0]
    if xi < 0:
        index, xi = index[:, abs(xi):], 0
    if xf > image.shape[1]:
        index, xf = index[:, : index.shape[1] - (xf - image.shape[1])], image.shape[1]
    roi_m, roi_i = mask[yi:yf, xi:xf], image[yi:yf, xi:xf]
    if roi_i.size and index.shape == roi_i.shape:
        roi_m[index] = (((roi_i[index] >= thresh[0]) & (roi_i[index] <= thresh[1])) * 253) + 1


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


def main():
    n = args.size
    L.require_device()
    img = synth_v512((n, n, n))
    mask = np.zeros((n + 1,) * 3, np.uint8)
    slice_.do_threshold_to_all_slices(mask, img, BONE)
    for ax in range(3):  # every slice of every orientation up to date, as after the viewer has shown them
        idx = [slice(0, 1)] * 3
        idx[ax] = slice(1, None)
        mask[tuple(idx)] = 1
    mid = n // 2
    bound = {}

    def next_use(ori):
        slice_.project(slab(mask[1:, 1:, 1:], ori, mid), ORIENTATIONS.index(ori), slice_.PROJECTION_MaxIP)

    def kernel_route(ori, index, positions):
        slice_.edit_mask_stroke(mask, img, ori, mid, index, positions, slice_.BRUSH_THRESH, EDITION)
        next_use(ori)

    def numpy_route(ori, index, positions):
        view = slice_view(mask[1:, 1:, 1:], ori, mid)
        b = np.array(view)
        image = slice_view(img, ori, mid)
        for pos in positions:
            numpy_dab(b, image, index, pos, EDITION)
        view[...] = b
        flag = [0, 0, 0]
        flag[ORIENTATIONS.index(ori)] = mid + 1
        mask[tuple(flag)] = 2
        if "mask" in bound:
            bound["mask"].touch(view)
            bound["mask"].touch(mask[tuple(slice(f, f + 1) for f in flag)])
        next_use(ori)

    res = {}
    for half in ("unbound", "bound"):
        if half == "bound":
            t0 = time.perf_counter()
            bound["image"], bound["mask"] = slice_.bind_image(img), mask_mod.bind_matrix(mask)
            res["bind_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        for radius in (15, 100):
            index = cursor.cursor_pixels(cursor.BRUSH_CIRCLE, radius, "px")
            for ori in ORIENTATIONS:
                stroke = [(n * 0.2 + k * n * 0.6 / max(args.dabs - 1, 1), n * 0.3 + k * n * 0.4 / max(args.dabs - 1, 1)) for k in range(args.dabs)]
                for what, positions in (("stroke of %d dabs" % args.dabs, stroke), ("single dab", stroke[:1])):
                    key = "radius %d px, %s, %s" % (radius, ori, what)
                    entry = res.setdefault(key, {})
                    entry["stroke kernel, %s" % half] = timeit(lambda: kernel_route(ori, index, positions))
                    entry["numpy%s, %s" % (" + touch" if half == "bound" else "", half)] = timeit(lambda: numpy_route(ori, index, positions))
    for r in bound.values():
        r.release()
    print(json.dumps({"size": "%d^3 image, %d^3 mask" % (n, n + 1), "device": L.device_name(),
                      "protocol": "wall clock around the Python calls (stroke + the next use of the slice, a one-slice MaxIP), median of %d "
                                  "after one warm-up (min / max beside it); moved_per_call: bytes the library's copy helpers moved"
                                  % args.reps, "results": res}, indent=1))


if __name__ == "__main__":
    main()
