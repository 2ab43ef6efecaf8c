"""Device times of the mask 3-D preview (k_maskren.hip) on the resident synth_v512 volume thresholded at (226, 3071): the
macro cells, the render at 1024^2 and 2048^2 from the Front and Iso views in both modes with the samples taken and
skipped, and one slider step (threshold + cells + render at 1024^2, synchronised wall clock).  The comparator is the
only way to this picture without the feature: the mask downloaded, widened to int16 and uploaded as an image (wall
clock), then ivx_dev_volren_prepare / _cells / _render with the same table and camera on the dense field.  HIP events,
2 warm-ups, median of 5.
python tools/bench_mask_preview.py [n] [--out profiles/bench_mask_preview_512.json]"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from bench import synth_v512  # noqa: E402
from invesalius3_amd import _lib as L  # noqa: E402
from invesalius3_amd import volume as V  # noqa: E402
from invesalius3_amd import volume_mask as VM  # noqa: E402
from invesalius3_amd.device import DeviceBuffer, DeviceVolume, c64  # noqa: E402

WARM, REPS = 2, 5
SPACING = (0.5, 0.5, 0.5)
THRESHOLD = (226, 3071)
COLOUR = (0.0, 1.0, 0.0)


def timed(vol, name, fn):
    for _ in range(WARM):
        fn()
    vol.sync()
    vol.timer.collect()  # drops (and recycles) the warm-up spans
    for _ in range(REPS):
        with vol.timer.span(name):
            fn()
    vol.sync()
    return statistics.median(vol.timer.collect()[name])


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 512
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/bench_mask_preview_%d.json" % n
    img = np.ascontiguousarray(synth_v512((n, n, n)))
    res = {"volume": [n, n, n], "spacing": list(SPACING), "threshold": list(THRESHOLD), "device": L.device_name(),
           "warmup": WARM, "reps": REPS, "render": []}
    lib = L.lib()
    with DeviceVolume(img, spacing=SPACING) as vol:
        shape = L.i64(vol.shape)
        dense = L.i64([vol.dy * vol.dx, vol.dx, 1])
        res["threshold_ms"] = round(timed(vol, "thr", lambda: vol.threshold(*THRESHOLD)), 4)
        cells = vol._maskren_cells(1)
        res["cells_ms"] = round(timed(vol, "cells", lambda: L.check(lib.ivx_dev_maskren_cells(
            vol.mask_bytes(), shape, dense, 1, 1, c64(0), c64(-1), cells.ptr, vol.stream))), 4)
        res["cells_slab_16_ms"] = round(timed(vol, "cells16", lambda: L.check(lib.ivx_dev_maskren_cells(
            vol.mask_bytes(), shape, dense, 1, 1, c64(n // 2), c64(n // 2 + 16), cells.ptr, vol.stream))), 4)
        # the comparator's field: download, widen on the host, upload as an image (the parent commit has no other way)
        t = time.perf_counter()
        mask = vol.download_mask()
        wide = mask.astype(np.int16)
        cmp_vol = DeviceVolume(wide, spacing=SPACING)
        cmp_vol.sync()
        res["comparator_widen_wall_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        res["mask_voxels"] = int(np.count_nonzero(mask))
        del mask, wide
        field = DeviceBuffer(vol.n * 2)
        cshape = [-(-s // V.CELL) for s in vol.shape]
        ccells = DeviceBuffer(int(np.prod(cshape)) * 4)
        res["comparator_prepare_ms"] = round(timed(cmp_vol, "prep", lambda: L.check(lib.ivx_dev_volren_prepare(
            cmp_vol.image.raw, shape, 0, 0, field.ptr, None, cmp_vol.stream))), 4)
        res["comparator_cells_ms"] = round(timed(cmp_vol, "cells", lambda: L.check(lib.ivx_dev_volren_cells(
            field.ptr, shape, ccells.ptr, cmp_vol.stream))), 4)
        for size in (1024, 2048):
            for view in ("front", "iso"):
                for mode in VM.MODES:
                    vol.render_mask_preview(COLOUR, view, (size, size), mode=mode)
                    stats = dict(vol.last_render_stats)
                    cam = V.camera_for_view(view, vol.shape, vol.spacing, (size, size))
                    setup = VM.render_setup(COLOUR, mode, cam, vol.spacing)
                    p = V.volren_params(setup, vol.spacing)
                    tb, outd, nb = vol._mp_table, vol._mp_out, VM.N_TABLE * 16
                    iso = int(setup["iso"])

                    def run():
                        L.check(lib.ivx_dev_maskren_render(vol.mask_bytes(), cells.ptr, shape, dense, 1, 1, iso, tb.ptr,
                                                           tb.at(nb), ctypes.byref(p), outd.ptr, None, None, vol.stream))
                    ms = timed(vol, "render", run)
                    rec = {"mode": mode, "view": view, "size": size, "ms": round(ms, 4),
                           "mrays_per_s": round(size * size / ms / 1e3, 1), "samples": stats["samples"],
                           "skipped": stats["skipped"], "rays_hit": stats["rays_hit"],
                           "early_fraction": round(stats["early"] / max(stats["rays_hit"], 1), 4)}
                    if mode == "composite":
                        # the same table, alpha and camera through the uint16 renderer (dense field, no flag planes)
                        rgba, prefix = VM.device_tables(setup)
                        alpha = np.ascontiguousarray(setup["alpha"], np.float32)
                        ctb = DeviceBuffer(rgba.nbytes + alpha.nbytes + prefix.nbytes)
                        ctb.upload(np.concatenate([rgba.view(np.uint8).ravel(), alpha.view(np.uint8).ravel(),
                                                   prefix.view(np.uint8).ravel()]))
                        cst = DeviceBuffer(32)
                        cst.zero(cmp_vol.stream, 32)
                        cout = DeviceBuffer(size * size * 16)

                        def crun(st=None):
                            L.check(lib.ivx_dev_volren_render(field.ptr, ccells.ptr, shape, ctb.ptr, ctb.at(rgba.nbytes),
                                                              ctb.at(rgba.nbytes + alpha.nbytes), ctypes.byref(p), cout.ptr,
                                                              st, cmp_vol.stream))
                        crun(cst.ptr)
                        cmp_vol.sync()
                        cs = cst.download((4,), np.uint64)
                        rec["comparator_ms"] = round(timed(cmp_vol, "crender", crun), 4)
                        rec["comparator_samples"], rec["comparator_skipped"] = int(cs[0]), int(cs[1])
                        rec["ratio_to_comparator"] = round(ms / rec["comparator_ms"], 4)
                        for b in (ctb, cst, cout):
                            b.close()
                    res["render"].append(rec)
                    print(json.dumps(rec), flush=True)
        for b in (field, ccells):
            b.close()
        cmp_vol.close()
        # one slider step: threshold, cells, render, synchronised; what a user feels
        for mode in VM.MODES:
            walls = []
            for k in range(WARM + REPS):
                t = time.perf_counter()
                vol.threshold(THRESHOLD[0] + k, THRESHOLD[1])
                vol.render_mask_preview(COLOUR, "iso", (1024, 1024), mode=mode, download=False)
                vol.sync()
                walls.append((time.perf_counter() - t) * 1e3)
            res["slider_step_1024_iso_%s_wall_ms" % mode] = round(statistics.median(walls[WARM:]), 4)
    m = np.zeros((n + 1, n + 1, n + 1), np.uint8)
    m[1:, 1:, 1:] = ((img >= THRESHOLD[0]) & (img <= THRESHOLD[1])) * 255
    walls = []
    for k in range(3):
        t = time.perf_counter()
        VM.mask_preview(m, SPACING, COLOUR, "iso", (1024, 1024), "iso")
        walls.append((time.perf_counter() - t) * 1e3)
    res["host_entry_1024_iso_ms"] = round(statistics.median(walls[1:]), 3)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "render"}))


if __name__ == "__main__":
    main()
