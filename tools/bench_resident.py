#!/usr/bin/env python3
"""Host-level entry points with the project's arrays bound (resident.bind) against the same calls unbound, in one run:
the calls of tools/bench_host.py that take the image or the mask matrix, each timed both ways (wall clock around the
Python call, median of five after a warm-up, min / max beside it) with the bytes the library's copy helpers moved per
call beside each time -- the counters say what the binding removed, the clock what that was worth.  Plus the short-row
view the binding serves with the gather kernel (a sagittal slab, k = 1) against the host row gather it replaces.

    python tools/bench_resident.py                    # 512^3, both halves
    python tools/bench_resident.py --unbound-only --tree OTHER_CHECKOUT
        the unbound half alone on another build of the package (the parent commit: no-regression figure, same box, same run)
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
p.add_argument("--unbound-only", action="store_true")
p.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
               help="checkout whose invesalius3_amd and bench.py are measured (default: this one)")
args = p.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

from scipy.ndimage import generate_binary_structure  # noqa: E402

from bench import BONE, synth_v512  # noqa: E402
from invesalius3_amd import _lib as L  # noqa: E402
from invesalius3_amd import invesalius_rs as rs, slice_  # noqa: E402

try:
    from invesalius3_amd import resident
except ImportError:  # a build from before the feature: its unbound half is all there is to measure
    resident = None
    args.unbound_only = True


def counters():
    return resident.transfer_stats() if resident is not None else {}


def timeit(fn, before=None):
    t, moved = [], None
    for i in range(args.reps + 1):
        if before is not None:
            before()
        c0 = counters()
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i:
            t.append(dt)
            moved = {k: v - c0[k] for k, v in counters().items()}  # (of the last call: they are all alike)
    out = {"ms": round(float(np.median(t)) * 1e3, 3), "min_ms": round(min(t) * 1e3, 3), "max_ms": round(max(t) * 1e3, 3), "calls": len(t)}
    if moved is not None:
        out["moved_per_call"] = moved
    return out


def main():
    n = args.size
    L.require_device()
    img = synth_v512((n, n, n))
    mask = np.zeros((n + 1,) * 3, np.uint8)
    z, y, x = (int(v) for v in np.unravel_index(int(np.argmax(img)), img.shape))
    s26 = generate_binary_structure(3, 3)
    out = np.zeros(img.shape, np.uint8)
    view = mask[1:, 1:, 1:]
    o2 = np.zeros((n, n), np.int16)
    bound = {}

    def flags_reset():  # the reference clears the flags of the slices it wants redone; a bound matrix is told, cell by cell
        mask[1:, 0, 0] = 0
        if "mask" in bound:
            for k in range(1, n + 1):
                bound["mask"].touch(mask[k, :1, :1])

    def view_reset():  # (a library call, so that a bound matrix follows without a touch)
        rs.floodfill_threshold_inplace(view, [(x, y, z)], 254, 254, 255, s26)

    calls = [
        ("do_threshold_to_all_slices (strided mask, preserve rule)", lambda: slice_.do_threshold_to_all_slices(mask, img, BONE), flags_reset),
        ("floodfill_threshold_inplace (mask view [1:,1:,1:])", lambda: rs.floodfill_threshold_inplace(view, [(x, y, z)], 253, 255, 254, s26),
         view_reset),
        ("floodfill_threshold (26-conn, dense out, unbound out)", lambda: rs.floodfill_threshold(img, [(x, y, z)], BONE[0], BONE[1], 1, s26, out),
         lambda: out.fill(0)),
        ("project MaxIP axis 0", lambda: slice_.project(img, 0, slice_.PROJECTION_MaxIP), None),
        ("mida axis 0", lambda: rs.mida(img, 0, 300, 600, o2), None),
        ("project MaxIP of an axial slab, k = 5", lambda: slice_.project(img[n // 2:n // 2 + 5], 0, slice_.PROJECTION_MaxIP), None),
        ("project MaxIP of a coronal slab, k = 5", lambda: slice_.project(img[:, n // 2:n // 2 + 5], 1, slice_.PROJECTION_MaxIP), None),
        ("project MaxIP of a sagittal slab, k = 5", lambda: slice_.project(img[:, :, n // 2:n // 2 + 5], 2, slice_.PROJECTION_MaxIP), None),
        ("project MaxIP of a sagittal slab, k = 1 (short rows: host row gather unbound, gather kernel bound)",
         lambda: slice_.project(img[:, :, n // 2:n // 2 + 1], 2, slice_.PROJECTION_MaxIP), None),
    ]
    res = {"unbound": {}, "bound": {}}
    for name, fn, before in calls:
        res["unbound"][name] = timeit(fn, before)
    if not args.unbound_only:
        t0 = time.perf_counter()
        bound["image"] = slice_.bind_image(img)
        from invesalius3_amd import mask as mask_mod
        bound["mask"] = mask_mod.bind_matrix(mask)
        res["bind_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        for name, fn, before in calls:
            res["bound"][name] = timeit(fn, before)
        res["registrations"] = {k: r.stats() for k, r in bound.items()}
        for r in bound.values():
            r.release()
    else:
        del res["bound"]
    print(json.dumps({"size": "%d^3" % n, "device": L.device_name(),
                      "protocol": "wall clock around the Python call, median of %d after one warm-up (min / max beside it); "
                                  "moved_per_call: bytes the library's copy helpers moved during one call" % args.reps,
                      "results": res}, indent=1))


if __name__ == "__main__":
    main()
