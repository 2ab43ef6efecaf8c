"""Device times of the surface visibility tool (k_meshvis.hip) on the bench surface: synth_v512 thresholded at (226, 3071), its
indexed mesh resident in HBM, the reference's six views at 800 x 800.  Reported in microseconds: the bounds, the raster per view
(clear, lane-per-triangle kernel and workgroup-per-triangle kernel apart), the point test over the six views (flags minus the
six rasters is in `points_us`), the selection, the whole tool on the resident mesh, and the host-array call with PCIe (wall clock).
There is no reference timing to put beside these: VTK is not installed, and the numpy restatement of tests/ is a checker, not a
baseline.  HIP events, 2 warm-ups, median of 5.
python tools/bench_surface_visibility.py [n] [--out profiles/bench_surface_visibility_512.json]"""
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
from invesalius3_amd import polydata_utils as pu  # noqa: E402
from invesalius3_amd.device import DeviceBuffer, DeviceVolume, c64  # noqa: E402

WARM, REPS = 2, 5
SPACING = (0.5, 0.5, 0.5)
THRESHOLD = (226, 3071)
CLEAR, SMALL, BIG = 1, 2, 4  # IVX_RASTER_*


def timed(vol, name, fn):
    for _ in range(WARM):
        fn()
    vol.sync()
    vol.timer.collect()  # drops (and recycles) the warm-up spans
    for _ in range(REPS):
        with vol.timer.span(name):
            fn()
    vol.sync()
    return round(statistics.median(vol.timer.collect()[name]) * 1e3, 2)  # ms -> us


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 512
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/bench_surface_visibility_%d.json" % n
    img = np.ascontiguousarray(synth_v512((n, n, n)))
    lib = L.lib()
    res = {"volume": [n, n, n], "spacing": list(SPACING), "threshold": list(THRESHOLD), "size": list(pu.SIZE),
           "device": L.device_name(), "warmup": WARM, "reps": REPS, "unit": "us"}
    with DeviceVolume(img, spacing=SPACING) as vol:
        vol.threshold(*THRESHOLD)
        mesh = pu.DeviceMesh.from_volume(vol, vol.marching_cubes_indexed(from_binary=True, fill_border_holes=True))
        nv, nt = mesh.nverts, mesh.ntris
        res["vertices"], res["triangles"] = nv, nt
        b6 = DeviceBuffer(64)
        res["bounds_us"] = timed(vol, "bounds", lambda: L.check(lib.ivx_dev_mesh_bounds(mesh.verts.ptr, c64(nv), b6.ptr, vol.stream)))
        b6.close()
        views = pu.views_for_positions(mesh.bounds())
        cviews = pu._c_views(views)
        depth = DeviceBuffer(pu.SIZE[0] * pu.SIZE[1] * 4)

        def stage(k, bits):
            return lambda: L.check(lib.ivx_dev_mesh_depth_raster(mesh.verts.ptr, c64(nv), mesh.faces.ptr, c64(nt), ctypes.byref(cviews[k]),
                                                                 bits, depth.ptr, vol.stream))
        res["raster"] = []
        for k in range(len(views)):
            rec = {"view": k}
            # the small kernel appends to the queue: clear it (untimed) before every timed run of it
            for _ in range(WARM):
                stage(k, CLEAR)()
                stage(k, SMALL)()
            vol.sync()
            vol.timer.collect()
            for _ in range(REPS):
                stage(k, CLEAR)()
                with vol.timer.span("small"):
                    stage(k, SMALL)()
            vol.sync()
            rec["small_us"] = round(statistics.median(vol.timer.collect()["small"]) * 1e3, 2)
            rec["big_us"] = timed(vol, "big", stage(k, BIG))  # (the queue the last small run left)
            rec["clear_us"] = timed(vol, "clear", stage(k, CLEAR))
            rec["all_us"] = timed(vol, "all", stage(k, CLEAR | SMALL | BIG))
            vol.sync()
            d = depth.download((pu.SIZE[1], pu.SIZE[0]), np.float32)
            rec["covered_pixels"] = int(np.count_nonzero(d < 1.0))
            res["raster"].append(rec)
            print(json.dumps(rec), flush=True)
        depth.close()
        flags = DeviceBuffer(nv + 16)
        res["flags_six_views_us"] = timed(vol, "flags", lambda: L.check(lib.ivx_dev_mesh_visible_points(
            mesh.verts.ptr, c64(nv), mesh.faces.ptr, c64(nt), cviews, len(views), flags.ptr, vol.stream)))
        res["points_us"] = round(res["flags_six_views_us"] - sum(r["all_us"] for r in res["raster"]), 2)
        vol.sync()
        res["visible_points"] = int(np.count_nonzero(flags.download((nv,), np.uint8)))
        ov, of = DeviceBuffer(nv * 12 + 16), DeviceBuffer(nt * 12 + 16)
        n1, n2 = ctypes.c_int64(0), ctypes.c_int64(0)
        res["select_us"] = timed(vol, "select", lambda: L.check(lib.ivx_dev_mesh_select_points(
            mesh.verts.ptr, c64(nv), mesh.faces.ptr, c64(nt), flags.ptr, 0, ov.ptr, c64(nv), of.ptr, c64(nt), ctypes.byref(n1),
            ctypes.byref(n2), vol.stream)))
        res["kept_vertices"], res["kept_triangles"] = n1.value, n2.value
        for b in (flags, ov, of):
            b.close()

        def tool():
            pu.RemoveNonVisibleFaces(mesh).close()
        res["tool_resident_us"] = timed(vol, "tool", tool)  # bounds + download of 24 bytes + cameras + flags + selection + buffers
        walls = []
        for _ in range(WARM + REPS):
            t = time.perf_counter()
            tool()
            vol.sync()
            walls.append((time.perf_counter() - t) * 1e6)
        res["tool_resident_wall_us"] = round(statistics.median(walls[WARM:]), 1)
        verts, faces = mesh.download()
    walls = []
    for _ in range(1 + 3):
        t = time.perf_counter()
        pu.RemoveNonVisibleFaces(verts, faces)
        walls.append((time.perf_counter() - t) * 1e6)
    res["host_arrays_wall_us"] = round(statistics.median(walls[1:]), 1)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "raster"}))


if __name__ == "__main__":
    main()
