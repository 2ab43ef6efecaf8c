#!/usr/bin/env python3
"""The image geometry tools -- flip, swap axes, gantry tilt -- on a 512^3 int16 image with one 513^3 mask:

  kernel                  the device form alone on a resident block, HIP events around it (what the byte model speaks of)
  tool, bound             slice_.flip_volume / swap_volume_axes / fix_gantry_tilt on the bound image and mask
  tool, unbound           the same call on arrays nobody bound: upload, compute, download
  numpy + touch, bound    the only route without the feature: numpy (scipy for the tilt) on the host arrays, the mask
                          cleared with numpy, `Resident.touch` on both -- which uploads them again at the next use; after a
                          swap the new arrays are bound afresh (one upload each)
  numpy, unbound          the same without a binding

Every timed window ends with the same next use, the slab MaxIP get_image_slice computes (four axial slices, taken on a view
of the matrix so that a bound image is read from its mirror), so that the upload a touch only schedules is paid inside it.
The tilt's scipy side runs on a 64-slice sub-volume of the same image and is reported as that: FixGantryTilt takes a
whole-volume minimum per slice, which makes it quadratic in the number of slices; nothing is extrapolated.  Wall clock
around the Python calls (they end synchronised), median of five after a warm-up, min / max and the bytes the library's copy
helpers moved per call beside it.

    python tools/bench_image_tools.py > profiles/bench_image_tools_512.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

p = argparse.ArgumentParser()
p.add_argument("--size", type=int, default=512)
p.add_argument("--reps", type=int, default=5)
p.add_argument("--scipy-slices", type=int, default=64)
args = p.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import synth_v512  # noqa: E402
from invesalius3_amd import _lib as L  # noqa: E402
from invesalius3_amd import resident, slice_  # noqa: E402
from invesalius3_amd import mask as mask_mod  # noqa: E402
from invesalius3_amd.device import DeviceBuffer, Timer  # noqa: E402

SPACING = (0.5, 0.5, 1.0)
SWAPS = ((2, 1), (2, 0), (1, 0))
TILTS = (0.5, 11.5, -20.0)
REV = (np.s_[::-1], np.s_[:, ::-1], np.s_[:, :, ::-1])


def stats(t, moved=None):
    out = {"ms": round(float(np.median(t)) * 1e3, 3), "min_ms": round(min(t) * 1e3, 3), "max_ms": round(max(t) * 1e3, 3), "calls": len(t)}
    if moved is not None:
        out["moved_per_call"] = moved
    return out


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
    return stats(t, moved)


def next_use(matrix):
    mid = matrix.shape[0] // 2
    slice_.project(matrix[mid:mid + 4], 0, slice_.PROJECTION_MaxIP)


def kernels(img):
    """the device forms alone, HIP events on one stream"""
    lib = L.lib()
    n = img.shape[0]
    c = ctypes.c_int64
    s = ctypes.c_void_p()
    L.check(lib.ivx_stream_create(ctypes.byref(s)))
    timer = Timer(s)
    a, b = DeviceBuffer(img.nbytes), DeviceBuffer(img.nbytes)
    nb = ctypes.c_size_t(0)
    L.check(lib.ivx_image_tilt_scratch_bytes(c(n), c(n), c(n), ctypes.byref(nb)))
    scratch = DeviceBuffer(nb.value)
    a.upload(img)
    out = {}

    def run(name, fn):
        for _ in range(args.reps + 1):
            with timer.span(name):
                L.check(fn(), name)
            L.check(lib.ivx_stream_synchronize(s))
        out[name] = stats([v * 1e-3 for v in timer.collect()[name][1:]])

    for axis in range(3):
        run("flip %d" % axis, lambda: lib.ivx_dev_image_flip(a.ptr, c(n), c(n), c(n), 2, axis, s))
    for x, y in SWAPS:
        run("swap (%d, %d)" % (x, y), lambda: lib.ivx_dev_image_swap_axes(a.ptr, c(n), c(n), c(n), 2, x, y, b.ptr, s))
    for tilt in TILTS:
        shifts = slice_.gantry_tilt_shifts(n, SPACING, tilt)
        # (the span holds the two launches and the host's look at the minima between them)
        run("tilt %g" % tilt, lambda: lib.ivx_dev_image_fix_gantry_tilt(a.ptr, c(n), c(n), c(n), L.ptr(shifts), scratch.ptr,
                                                                      ctypes.c_size_t(scratch.nbytes), None, s))
    for buf in (a, b, scratch):
        buf.close()
    L.check(lib.ivx_stream_destroy(s))
    return out


def main():
    n = args.size
    L.require_device()
    img0 = synth_v512((n, n, n))
    res = {"kernel": kernels(img0)}
    state = {}

    def fresh(bound):
        for r in state.get("bound", []):
            r.release()
        state["img"], state["mask"] = img0.copy(), np.zeros((n + 1,) * 3, np.uint8)
        state["bound"] = [slice_.bind_image(state["img"]), mask_mod.bind_matrix(state["mask"])] if bound else []

    def rebind():
        """what swap leaves behind: the package's new bindings in place of the old ones"""
        state["bound"] = [r for r in (resident.find(state["img"]), resident.find(state["mask"])) if r is not None]

    def tool_flip(axis):
        slice_.flip_volume(state["img"], axis, masks=[state["mask"]])
        next_use(state["img"])

    def tool_swap(axes):
        state["img"], _, (state["mask"],), _ = slice_.swap_volume_axes(state["img"], axes, SPACING, masks=[state["mask"]])
        if state["bound"]:
            rebind()
        next_use(state["img"])

    def tool_tilt(tilt):
        slice_.fix_gantry_tilt(state["img"], SPACING, tilt, masks=[state["mask"]])
        next_use(state["img"])

    def clear_mask_numpy():
        state["mask"][:] = 0
        if state["bound"]:
            state["bound"][1].touch()

    def numpy_flip(axis):
        m = state["img"]
        m[:] = m[REV[axis]]
        if state["bound"]:
            state["bound"][0].touch()
        clear_mask_numpy()
        next_use(m)

    def numpy_swap(axes):
        new = np.array(state["img"].swapaxes(*axes))
        new_mask = np.zeros(tuple(s + 1 for s in new.shape), np.uint8)
        was_bound = bool(state["bound"])
        for r in state["bound"]:
            r.release()
        state["img"], state["mask"] = new, new_mask
        state["bound"] = [slice_.bind_image(new), mask_mod.bind_matrix(new_mask)] if was_bound else []
        next_use(new)

    def scipy_tilt(tilt):
        from scipy.ndimage import shift
        m = state["sub"]
        for k, s in enumerate(slice_.gantry_tilt_shifts(m.shape[0], SPACING, tilt)):
            m[k] = shift(m[k], (s, 0), cval=m.min())
        if state["sub_bound"]:
            state["sub_bound"].touch()
        clear_mask_numpy()
        next_use(m)

    for half in ("unbound", "bound"):
        bound = half == "bound"
        label_np = "numpy + touch, bound" if bound else "numpy, unbound"
        for axis in range(3):
            entry = res.setdefault("flip %d" % axis, {})
            fresh(bound)
            entry["tool, %s" % half] = timeit(lambda: tool_flip(axis))
            fresh(bound)
            entry[label_np] = timeit(lambda: numpy_flip(axis))
        for axes in SWAPS:
            entry = res.setdefault("swap (%d, %d)" % axes, {})
            fresh(bound)
            entry["tool, %s" % half] = timeit(lambda: tool_swap(axes))
            fresh(bound)
            entry[label_np] = timeit(lambda: numpy_swap(axes))
        for tilt in TILTS:
            entry = res.setdefault("tilt %g" % tilt, {})
            fresh(bound)
            entry["tool, %s" % half] = timeit(lambda: tool_tilt(tilt))
            sub = img0[:args.scipy_slices].copy()
            state["sub"], state["sub_bound"] = sub, (slice_.bind_image(sub) if bound else None)
            key = ("scipy + touch, bound" if bound else "scipy, unbound") + ", %d-slice sub-volume" % sub.shape[0]
            entry[key] = timeit(lambda: scipy_tilt(tilt))
            sub_tool = img0[:args.scipy_slices].copy()
            entry["tool, unbound, the same %d-slice sub-volume" % sub.shape[0]] = timeit(
                lambda: (slice_.fix_gantry_tilt(sub_tool, SPACING, tilt), next_use(sub_tool)))
            if state["sub_bound"]:
                state["sub_bound"].release()
    for r in state.get("bound", []):
        r.release()
    print(json.dumps({"size": "%d^3 int16 image, %d^3 mask" % (n, n + 1), "device": L.device_name(), "spacing": list(SPACING),
                      "protocol": "kernel: HIP events around the device form, median of %d after a warm-up; everything else: wall clock "
                                  "around the Python calls plus the next use (a 4-slice axial MaxIP of the matrix), median of %d after a "
                                  "warm-up (min / max beside it); moved_per_call: bytes the library's copy helpers moved; repeated tilts "
                                  "work on their own output" % (args.reps, args.reps), "results": res}, indent=1))


if __name__ == "__main__":
    main()
