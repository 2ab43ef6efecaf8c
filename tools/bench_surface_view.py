"""Device times of the surface view (k_surfview.hip) on the bench surface: synth_v512 thresholded at (226, 3071), the largest
part of its indexed mesh resident in HBM with the point normals of surface_process.point_normals.  Front and Iso, 1024^2 and
2048^2, one opaque surface and a translucent-over-opaque pair (the part at transparency 0.5 over a copy of itself shrunk to 0.8
about its centre).  Reported in microseconds: the raster's three stages apart and together, the resolve, the whole
device-resident call (float32 picture left on the device), and the host call with upload, download and PNG (wall clock).
The yardstick, taken in the same run: the unchanged ivx_dev_mesh_depth_raster -- the 32-bit atomic form of the same walk -- on
the same mesh and size from the same side.  HIP events, 2 warm-ups, median of 5.
python tools/bench_surface_view.py [n] [--out profiles/bench_surface_view_512.json]"""
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")
from bench import synth_v512  # noqa: E402
from invesalius3_amd import _lib as L  # noqa: E402
from invesalius3_amd import polydata_utils as pu  # noqa: E402
from invesalius3_amd import surface_process as sp  # noqa: E402
from invesalius3_amd import surface_view as SV  # noqa: E402
from invesalius3_amd import volume as V  # noqa: E402
from invesalius3_amd.device import DeviceBuffer, DeviceVolume, c64  # noqa: E402

WARM, REPS = 2, 5
SPACING = (0.5, 0.5, 0.5)
THRESHOLD = (226, 3071)
CLEAR, SMALL, BIG = 1, 2, 4  # IVX_RASTER_*


def timed(vol, name, fn, before=None):
    """median device time of fn in us; `before` runs untimed ahead of every run"""
    for k in range(WARM + REPS):
        if k == WARM:
            vol.sync()
            vol.timer.collect()  # drops (and recycles) the warm-up spans
        if before is not None:
            before()
        if k < WARM:
            fn()
        else:
            with vol.timer.span(name):
                fn()
    vol.sync()
    return round(statistics.median(vol.timer.collect()[name]) * 1e3, 2)  # ms -> us


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 512
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/bench_surface_view_%d.json" % n
    img = np.ascontiguousarray(synth_v512((n, n, n)))
    lib = L.lib()
    res = {"volume": [n, n, n], "spacing": list(SPACING), "threshold": list(THRESHOLD), "device": L.device_name(), "warmup": WARM,
           "reps": REPS, "unit": "us", "runs": []}
    with DeviceVolume(img, spacing=SPACING) as vol:
        vol.threshold(*THRESHOLD)
        whole = pu.DeviceMesh.from_volume(vol, vol.marching_cubes_indexed(from_binary=True, fill_border_holes=True))
        part = whole.keep_largest()
        vol.sync()
        verts, faces = part.download()
        part.close()
        verts, faces, normals, _ = sp.point_normals(verts, faces)
        res["vertices"], res["triangles"] = len(verts), len(faces)
        centre = (verts.min(0).astype(np.float64) + verts.max(0).astype(np.float64)) / 2
        inner_verts = (centre + 0.8 * (verts.astype(np.float64) - centre)).astype(np.float32)
        mesh, inner = pu.DeviceMesh.upload(verts, faces, vol.stream), pu.DeviceMesh.upload(inner_verts, faces, vol.stream)
        d_normals = DeviceBuffer(normals.nbytes)
        d_normals.upload(normals)
        bounds = mesh.bounds()
        nv, nt = mesh.nverts, mesh.ntris
        for view in ("front", "iso"):
            for size in (1024, 2048):
                rec = {"view": view, "size": size}
                cam = SV.camera_for_bounds(view, bounds, (size, size))
                cc = SV._c_camera(cam)
                keys = DeviceBuffer(size * size * 8)

                def stage(bits):
                    return lambda: L.check(lib.ivx_dev_surface_raster(mesh.verts.ptr, c64(nv), mesh.faces.ptr, c64(nt), ctypes.byref(cc), bits,
                                                                      keys.ptr, vol.stream))
                # the small kernel appends to the queue: clear (untimed) before every run of it; big drains what the last small left
                rec["small_us"] = timed(vol, "small", stage(SMALL), before=stage(CLEAR))
                rec["big_us"] = timed(vol, "big", stage(BIG))
                rec["clear_us"] = timed(vol, "clear", stage(CLEAR))
                rec["raster_us"] = timed(vol, "raster", stage(CLEAR | SMALL | BIG))
                keys.close()
                # the yardstick: the depth-only rasteriser of the visibility tool from the same side
                mview = pu._c_views(pu.views_for_positions(bounds, [V.VIEWS[view][1]], (size, size)))
                zbuf = DeviceBuffer(size * size * 4)
                rec["depth_raster_us"] = timed(vol, "zraster", lambda: L.check(lib.ivx_dev_mesh_depth_raster(
                    mesh.verts.ptr, c64(nv), mesh.faces.ptr, c64(nt), ctypes.byref(mview[0]), CLEAR | SMALL | BIG, zbuf.ptr, vol.stream)))
                zbuf.close()
                rec["raster_over_depth_raster"] = round(rec["raster_us"] / rec["depth_raster_us"], 3)
                for label, actors in (("one", [SV.SurfaceActor(mesh, normals=d_normals)]),
                                      ("pair", [SV.SurfaceActor(mesh, normals=d_normals, transparency=0.5),
                                                SV.SurfaceActor(inner, normals=d_normals, colour=SV.SURFACE_COLOUR[5])])):
                    with SV.Scene(actors, vol.stream) as scene:
                        def whole_call():
                            scene.invalidate()
                            scene.render(cam, (size, size), download=False)
                        rec[label + "_call_us"] = timed(vol, "call", whole_call)
                        rec[label + "_resolve_us"] = timed(vol, "resolve", lambda: scene.render(cam, (size, size), download=False))
                        rec[label + "_resolve_rgba8_us"] = timed(vol, "resolve8", lambda: scene.render(cam, (size, size), rgba8=True, download=False))
                        ids = scene.render(cam, (size, size), ids=True)["ids"]
                        rec[label + "_covered_pixels"] = int(np.count_nonzero(ids[..., 0] >= 0))
                        walls = []
                        for _ in range(WARM + REPS):
                            t = time.perf_counter()
                            scene.render(cam, (size, size), rgba8=True)
                            walls.append((time.perf_counter() - t) * 1e6)
                        rec[label + "_resolve_download_wall_us"] = round(statistics.median(walls[WARM:]), 1)
                res["runs"].append(rec)
                print(json.dumps(rec), flush=True)
        for b in (mesh, inner, d_normals):
            b.close()
    # the host call: upload, raster, resolve, download, PNG
    png = os.path.join(tempfile.mkdtemp(prefix="bench_surface_view_"), "out.png")
    for size in (1024, 2048):
        walls, walls_png = [], []
        for _ in range(1 + 3):
            t = time.perf_counter()
            pic = SV.render_surfaces([SV.SurfaceActor(verts, faces, normals)], "iso", (size, size), rgba8=True)
            walls.append((time.perf_counter() - t) * 1e6)
            V.write_png(png, pic)
            walls_png.append((time.perf_counter() - t) * 1e6)
        res["host_call_%d_wall_us" % size] = round(statistics.median(walls[1:]), 1)
        res["host_call_png_%d_wall_us" % size] = round(statistics.median(walls_png[1:]), 1)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))


if __name__ == "__main__":
    main()
