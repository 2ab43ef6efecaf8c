"""Device times of the volume renderer (k_volren.hip) on the resident synth_v512 volume: prepare (shift and 0 / 1
smoothing passes), render at 1024^2 and 2048^2 for four presets at the Front and Iso views, a WW/WL change (bake, upload,
render), the histogram and the host entry.  HIP events, 2 warm-ups, median of 5; per render case the rays/s, the samples
taken and skipped and the share of rays terminated early.  Presets come from tests/golden/ref_volume.npz.
python tools/bench_volume.py [n] [--out profiles/bench_volume_512.json]"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from bench import synth_v512  # noqa: E402
import _volren_ref as R  # noqa: E402
from invesalius3_amd import _lib as L  # noqa: E402
from invesalius3_amd import volume as V  # noqa: E402
from invesalius3_amd.device import DeviceBuffer, DeviceVolume  # noqa: E402

WARM, REPS = 2, 5
SPACING = (0.5, 0.5, 0.5)
CASES = [("Bone + Skin", None), ("Gold Bone", None), ("Standard", None), ("MIP", None)]
TARGETS = {"shaded_1024_ms": 10.0, "mip_ms": 5.0, "frame_2048_ms": 30.0, "prepare_1pass_ms": 0.5, "histogram_ms": 0.2}


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
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/bench_volume_%d.json" % n
    presets, cluts, _ = R.fixture()
    img = np.ascontiguousarray(synth_v512((n, n, n)))
    res = {"volume": [n, n, n], "spacing": list(SPACING), "device": L.device_name(), "warmup": WARM, "reps": REPS,
           "prepare": {}, "render": [], "targets": TARGETS}
    lib = L.lib()
    with DeviceVolume(img, spacing=SPACING) as vol:
        shape = L.i64(vol.shape)
        outb, scratch = DeviceBuffer(vol.n * 2), DeviceBuffer(vol.n * 2)
        for passes in (0, 1):
            res["prepare"]["%d_pass" % passes] = timed(vol, "prep%d" % passes, lambda: L.check(lib.ivx_dev_volren_prepare(
                vol.image.raw, shape, 1024, passes, outb.ptr, scratch.ptr, vol.stream)))
        cshape = [-(-s // V.CELL) for s in vol.shape]
        cells = DeviceBuffer(int(np.prod(cshape)) * 4)
        res["prepare"]["cells"] = timed(vol, "cells", lambda: L.check(lib.ivx_dev_volren_cells(outb.ptr, shape, cells.ptr,
                                                                                                  vol.stream)))
        for b in (outb, scratch, cells):
            b.close()
        for name, _ in CASES:
            for size in (1024, 2048):
                for view in ("front", "iso"):
                    vol.render_volume(presets[name], view, (size, size), color_lists=cluts, download=True)
                    stats = dict(vol.last_render_stats)
                    setup, vr, tb = vol._vr_setup, vol._vr, vol._vr_table
                    p = V.volren_params(setup, vol.spacing)
                    nt = len(setup["alpha"])
                    outd = vol._vr_out

                    def run():
                        L.check(lib.ivx_dev_volren_render(vr["vol"].ptr, vr["cells"].ptr, shape, tb.ptr, tb.at(nt * 16),
                                                          tb.at(nt * 20), ctypes.byref(p), outd.ptr, None, vol.stream))
                    ms = timed(vol, "render", run)
                    rays = size * size
                    res["render"].append({
                        "preset": name, "view": view, "size": size, "ms": round(ms, 4), "mrays_per_s": round(rays / ms / 1e3, 1),
                        "shaded": bool(setup["shade"]), "mip": bool(setup["mip"]), "smoothing_passes": len(setup["kernels"]),
                        "samples": stats["samples"], "skipped": stats["skipped"], "rays_hit": stats["rays_hit"],
                        "early_fraction": round(stats["early"] / max(stats["rays_hit"], 1), 4)})
                    print(json.dumps(res["render"][-1]), flush=True)
        # a WW/WL drag: set_wwwl, bake, upload, render (wall clock, synchronised)
        p0 = presets["Bone + Skin"]
        vol.render_volume(p0, "iso", (1024, 1024), color_lists=cluts, download=False)
        vol.sync()
        walls = []
        for k in range(WARM + REPS):
            t = time.perf_counter()
            vol.render_volume(V.set_wwwl(p0, 300.0 + k, 200.0 + k, 0), "iso", (1024, 1024), color_lists=cluts, download=False)
            vol.sync()
            walls.append((time.perf_counter() - t) * 1e3)
        res["wwwl_change_1024_iso_ms"] = round(statistics.median(walls[WARM:]), 4)
        hist = DeviceBuffer(65536 * 8)
        lo, hi = vol._image_scale()
        res["histogram_ms"] = timed(vol, "hist", lambda: L.check(lib.ivx_dev_volren_histogram(
            vol.image.raw, ctypes.c_int64(vol.n), lo, hi - lo, hist.ptr, vol.stream)))
        hist.close()
    walls = []
    for k in range(3):
        t = time.perf_counter()
        V.volume_render(img, SPACING, presets["Bone + Skin"], "iso", (1024, 1024), color_lists=cluts)
        walls.append((time.perf_counter() - t) * 1e3)
    res["host_entry_1024_iso_ms"] = round(statistics.median(walls[1:]), 3)
    r = res["render"]
    shaded = [c["ms"] for c in r if c["shaded"] and c["size"] == 1024]
    res["target_check"] = {
        "shaded_1024_ms": max(shaded), "mip_ms": max(c["ms"] for c in r if c["mip"] and c["size"] == 1024),
        "frame_2048_ms": max(c["ms"] for c in r if c["size"] == 2048),
        "prepare_1pass_ms": res["prepare"]["1_pass"], "histogram_ms": res["histogram_ms"]}
    res["target_hit"] = {k: v <= TARGETS[k] for k, v in res["target_check"].items()}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("prepare", "wwwl_change_1024_iso_ms", "histogram_ms", "host_entry_1024_iso_ms",
                                          "target_check", "target_hit")}))


if __name__ == "__main__":
    main()
