#!/usr/bin/env python3
"""The 3-D mask editor on a bound (resident) mask matrix against the only route without it, in one run:

  editor        invesalius3_amd/mask3d_editor.py: the screen filter of all polygons in one launch, the cut and the stroke in
                place in the mirror, the changed planes copied to the host
  parent's way  what Mask3DEditorState does through the invesalius_rs call surface: polygon2mask_rs per polygon + numpy OR / .T
                (+ logical_not), two copies of the interior, mask_cut, the write-back into the matrix and Resident.touch();
                per dab brush_mask_rs on a contiguous copy of the interior, the write-back and touch()

Rows: the filter of 1 and of 8 polygons; one cut; a depth tick followed by the next preview picture; a drag of `--dabs` dabs
at brush size 30 followed by the next get_slices picture; end_brush_stroke; the kernels alone with HIP events.  512^3 image,
513^3 mask, thresholded at (226, 3071), 1024^2 viewport, Iso camera.  Wall clock around the Python calls (they end
synchronised), median of `--reps` after a warm-up, the bytes the library's copy helpers moved per call beside it.  The parent's
drag is measured on `--parent-dabs` dabs (every dab stages the volume both ways) and its per-dab time is reported.

    python tools/bench_mask3d_editor.py > profiles/bench_mask3d_editor_512.json
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
p.add_argument("--dabs", type=int, default=200)
p.add_argument("--parent-dabs", type=int, default=5)
p.add_argument("--viewport", type=int, default=1024)
args = p.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import BONE, synth_v512  # noqa: E402
from invesalius3_amd import _lib as L  # noqa: E402
from invesalius3_amd import history as H  # noqa: E402
from invesalius3_amd import invesalius_rs as rs  # noqa: E402
from invesalius3_amd import mask as mask_mod  # noqa: E402
from invesalius3_amd import mask3d_editor as M3  # noqa: E402
from invesalius3_amd import resident, slice_, slice_display, volume_mask  # noqa: E402
from invesalius3_amd import volume as V  # noqa: E402
from invesalius3_amd.device import DeviceBuffer, Timer  # noqa: E402

SPACING = (1.0, 1.0, 1.0)


def timeit(fn, reps=None, before=None):
    t, moved = [], None
    for i in range((reps or args.reps) + 1):
        if before is not None:
            before()
        c0 = resident.transfer_stats()
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i:
            t.append(dt)
            moved = {k: v - c0[k] for k, v in resident.transfer_stats().items()}
    return {"ms": round(float(np.median(t)) * 1e3, 3), "min_ms": round(min(t) * 1e3, 3), "max_ms": round(max(t) * 1e3, 3), "calls": len(t),
            "moved_per_call": moved}


def star(cx, cy, r, k, points=12):
    t = np.linspace(0, 2 * np.pi, points, endpoint=False) + 0.3 * k
    rr = r * (0.6 + 0.4 * (np.arange(points) % 2))
    return np.stack([cx + rr * np.cos(t), cy + rr * np.sin(t)], axis=1)


def main():
    n, vp = args.size, args.viewport
    L.require_device()
    img = synth_v512((n, n, n))
    mask = np.zeros((n + 1,) * 3, np.uint8)
    slice_.do_threshold_to_all_slices(mask, img, BONE)
    pristine = mask.copy()
    size = (vp, vp)
    cam = V.resolve_camera("iso", img.shape, SPACING, size)
    near, far = M3.default_clipping_range(cam)
    m, mv = M3.camera_matrices(cam, size, (near, far))
    polys8 = [star(vp * (0.2 + 0.08 * k), vp * (0.3 + 0.05 * k), vp * 0.07, k) for k in range(8)]
    one = [star(vp * 0.5, vp * 0.5, vp * 0.12, 0)]
    res_mask = mask_mod.bind_matrix(mask)
    res_img = slice_.bind_image(img)
    out = {}

    def reset():
        mask[...] = pristine
        res_mask.touch()
        H.snapshot(mask).close()  # the pending upload is paid here, outside the timed window

    # ---- filter
    def parent_filter(polys, mode):
        f = np.logical_or.reduce([rs.polygon2mask_rs(size, np.asarray(q, np.float64)) for q in polys]).T
        if mode == 0:
            np.logical_not(f, out=f)
        return f

    for name, polys in (("filter, 1 polygon", one), ("filter, 8 polygons", polys8)):
        out[name] = {"editor": timeit(lambda: M3.polygon_filter(size, polys, 1)), "parent's way": timeit(lambda: parent_filter(polys, 1))}
        assert np.array_equal(M3.polygon_filter(size, polys, 0), parent_filter(polys, 0))

    # ---- one cut
    def parent_cut(polys, depth, mode):
        f = parent_filter(polys, mode)
        _mat = mask[1:, 1:, 1:].copy()
        o = _mat.copy()
        rs.mask_cut(_mat, SPACING[0], SPACING[1], SPACING[2], depth, f, m, mv, o, mode)
        mask[1:, 1:, 1:] = o
        res_mask.touch()

    deep, half = far, near + (far - near) * 0.5
    out["one cut"] = {"editor": timeit(lambda: M3.cut_mask(mask, SPACING, one, size, m, mv, deep, 1), before=reset)}
    ours = mask.copy()
    out["one cut"]["parent's way"] = timeit(lambda: parent_cut(one, deep, 1), before=reset)
    assert np.array_equal(ours, mask)
    out["one cut"]["voxels cut"] = int((ours != pristine).sum())

    # ---- a depth tick and the next preview picture
    def preview():
        volume_mask.mask_preview(mask, SPACING, (0.0, 1.0, 0.0), cam, size, rgba8=True)

    out["depth tick + preview"] = {
        "editor": timeit(lambda: (M3.cut_mask(mask, SPACING, one, size, m, mv, half, 1), preview()), before=reset),
        "parent's way": timeit(lambda: (parent_cut(one, half, 1), preview()), before=reset)}

    # ---- a drag and the next slice picture
    t = np.linspace(0.0, 1.0, args.dabs)
    world = np.stack([n * (0.2 + 0.6 * t), -n * (0.3 + 0.4 * t), n * (0.35 + 0.3 * t)], axis=1)
    state = slice_display.DisplayState(window_width=2000.0, window_level=300.0)
    state.set_colour_table("Default ")
    image_range = (int(img.min()), int(img.max()))

    def picture():
        slice_.get_slices(img, mask, "AXIAL", n // 2, 1, state, image_range=image_range)

    def parent_drag(points):
        for wx, wy, wz in points:
            _mat = np.ascontiguousarray(mask[1:, 1:, 1:])
            rs.brush_mask_rs(_mat, None, SPACING, (wx + SPACING[0], -wy - SPACING[1], wz + SPACING[2]), 15.0, 1)
            mask[1:, 1:, 1:] = _mat
            res_mask.touch()

    key = "drag of %d dabs, size 30 + slice picture" % args.dabs
    out[key] = {"editor": timeit(lambda: (M3.brush_stroke(mask, None, SPACING, world, 30.0, 1), picture()), before=reset)}
    ours = mask.copy()
    pd = timeit(lambda: (parent_drag(world[:args.parent_dabs]), picture()), reps=2, before=reset)
    pd["dabs"] = args.parent_dabs
    pd["ms_per_dab"] = round(pd["ms"] / args.parent_dabs, 3)
    pd["extrapolated_ms_for_%d_dabs" % args.dabs] = round(pd["ms"] / args.parent_dabs * args.dabs, 1)
    out[key]["parent's way"] = pd
    out[key]["voxels erased"] = int((ours != pristine).sum())
    out["single dab, unbound matrix"] = {}
    free = pristine.copy()
    out["single dab, unbound matrix"]["editor"] = timeit(lambda: M3.brush_stroke(free, None, SPACING, world[:1], 30.0, 1), reps=3)

    def parent_dab_unbound():
        _mat = np.ascontiguousarray(free[1:, 1:, 1:])
        rs.brush_mask_rs(_mat, None, SPACING, (world[0][0] + 1.0, -world[0][1] - 1.0, world[0][2] + 1.0), 15.0, 1)
        free[1:, 1:, 1:] = _mat
    out["single dab, unbound matrix"]["parent's way"] = timeit(parent_dab_unbound, reps=3)
    del free

    # ---- the state machine's stroke bookkeeping
    hist = H.EditionHistory()
    st = M3.Mask3DEditorState(mask, SPACING, size, history=hist)
    st.setup_state()
    st.SetEditMode(1)

    def begin():
        reset()
        st.start_brush_stroke()
        st.brush_stroke(world[:20])
    out["end_brush_stroke"] = {"editor": timeit(st.end_brush_stroke, before=begin)}
    out["start_brush_stroke"] = {"editor": timeit(st.start_brush_stroke, before=reset)}
    st.close()
    hist.clear_history()

    # ---- the kernels alone, HIP events on the null stream
    reset()
    lib = L.lib()
    nbytes = mask.nbytes
    d_m, d_b, d_flags = DeviceBuffer(nbytes), DeviceBuffer(nbytes), DeviceBuffer(n + 1)
    d_m.upload_view(mask)
    d_b.upload_view(mask)
    d_flags.zero()
    pts, off = M3._pack_polygons(polys8)
    d_poly = DeviceBuffer(pts.nbytes + off.nbytes + 16)
    d_poly.upload(np.concatenate([off.view(np.uint8), pts.reshape(-1).view(np.uint8)]))
    d_f = DeviceBuffer(vp * vp)
    shape, strides = L.i64([n, n, n]), L.i64(mask.strides)
    centres = M3.brush_centres(world, SPACING)
    d_c = DeviceBuffer(centres.nbytes)
    d_c.upload(centres)
    eq = ctypes.c_int(0)
    kernels = {
        "filter, 8 polygons": lambda: lib.ivx_dev_m3e_filter(vp, vp, d_poly.at(off.nbytes), d_poly.at(0), 8, 1, d_f.ptr, None),
        "cut (re-run on the cut state: reads, projects what is left, stores nothing)":
            lambda: lib.ivx_dev_m3e_cut(d_m.ptr, shape, strides, M3._d3(SPACING), float(deep), d_f.ptr, vp, vp, L.ptr(m), L.ptr(mv), 1, d_flags.ptr, None),
        "stroke of %d dabs (re-run: tests, stores nothing)" % args.dabs:
            lambda: lib.ivx_dev_m3e_brush_stroke(d_m.ptr, None, shape, strides, M3._d3(SPACING), L.ptr(centres), d_c.ptr, len(centres), 15.0, 1,
                                                 d_flags.ptr, None),
        "equal": lambda: lib.ivx_dev_m3e_equal(d_m.ptr, d_b.ptr, nbytes, ctypes.byref(eq), None),
    }
    timer = Timer(None)
    out["kernels alone (HIP events, ms)"] = {}
    for name, fn in kernels.items():
        L.check(fn())
        L.synchronize()
        samples = []
        for _ in range(args.reps):
            with timer.span("k"):
                L.check(fn())
            samples.append(timer.collect()["k"][0])
        out["kernels alone (HIP events, ms)"][name] = {"ms": round(float(np.median(samples)), 4), "min_ms": round(min(samples), 4),
                                                       "max_ms": round(max(samples), 4)}
    # the first cut of the pristine mask, stores included: one sample per fresh copy
    first = []
    for _ in range(3):
        d_m.upload_view(pristine)
        with timer.span("k"):
            L.check(kernels["cut (re-run on the cut state: reads, projects what is left, stores nothing)"]())
        first.append(timer.collect()["k"][0])
    out["kernels alone (HIP events, ms)"]["cut of the pristine mask (stores included)"] = {"ms": round(float(np.median(first)), 4)}
    for b in (d_m, d_b, d_flags, d_poly, d_f, d_c):
        b.close()
    res_mask.release()
    res_img.release()
    print(json.dumps({"size": "%d^3 image, %d^3 mask, %d^2 viewport" % (n, n + 1, vp), "device": L.device_name(),
                      "mask_bytes": int(nbytes), "plane_bytes": int(mask[0].nbytes),
                      "protocol": "wall clock around the Python calls (they end synchronised), median of %d after one warm-up (min / max beside "
                                  "it); the mask is put back and its upload paid before every timed call; moved_per_call: bytes the library's "
                                  "copy helpers moved" % args.reps, "results": out}, indent=1))


if __name__ == "__main__":
    main()
