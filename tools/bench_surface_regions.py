"""Device times of the surface connectivity tools (k_meshparts.hip) on the bench surface: synth_v512 thresholded at
(226, 3071), its indexed mesh resident in HBM.  Reported in microseconds: keep-largest (the yardstick of the same run), the
region labels, the stable partition of the triangle labels with their low 8 / 16 / all bits as keys (1 / 2 / 3 radix passes: the
differences are the cost of a pass), the split (sizes call, filling call, both with their buffers), the per-part mass for a
sweep of the wave-per-part bound, the seeded select, the nearest point, and the host-array calls with PCIe (wall clock).
There is no reference timing to put beside these: VTK is not installed.  HIP events, 2 warm-ups, median of 5.
python tools/bench_surface_regions.py [n] [--out profiles/bench_surface_regions_512.json]"""
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
from invesalius3_amd import surface_process as sp  # noqa: E402
from invesalius3_amd.device import DeviceBuffer, DeviceVolume, c64  # noqa: E402

WARM, REPS = 2, 5
SPACING = (0.5, 0.5, 0.5)
THRESHOLD = (226, 3071)
SMALL_MAX = (64, 256, 1024, 4096, 16384, 1 << 30)


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


def wall(fn, warm=1, reps=3):
    out = []
    for _ in range(warm + reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e6)
    return round(statistics.median(out[warm:]), 1)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 512
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/bench_surface_regions_%d.json" % n
    img = np.ascontiguousarray(synth_v512((n, n, n)))
    lib = L.lib()
    res = {"volume": [n, n, n], "spacing": list(SPACING), "threshold": list(THRESHOLD), "device": L.device_name(), "warmup": WARM,
           "reps": REPS, "unit": "us"}
    with DeviceVolume(img, spacing=SPACING) as vol:
        vol.threshold(*THRESHOLD)
        mesh = pu.DeviceMesh.from_volume(vol, vol.marching_cubes_indexed(from_binary=True, fill_border_holes=True))
        nv, nt = mesh.nverts, mesh.ntris
        res["vertices"], res["triangles"] = nv, nt
        ov, of = DeviceBuffer(nv * 12 + 16), DeviceBuffer(nt * 12 + 16)
        n1, n2, nr = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        res["keep_largest_us"] = timed(vol, "keep", lambda: L.check(lib.ivx_dev_mesh_keep_largest(
            mesh.verts.ptr, c64(nv), mesh.faces.ptr, c64(nt), ov.ptr, c64(nv), of.ptr, c64(nt), ctypes.byref(n1), ctypes.byref(n2),
            ctypes.byref(nr), vol.stream)))
        res["regions"] = nr.value
        lab = DeviceBuffer(nt * 4 + 16)
        res["labels_us"] = timed(vol, "labels", lambda: L.check(lib.ivx_dev_mesh_region_labels(
            c64(nv), mesh.faces.ptr, c64(nt), lab.ptr, None, ctypes.byref(nr), None, vol.stream)))
        print(json.dumps({k: res[k] for k in ("triangles", "regions", "keep_largest_us", "labels_us")}), flush=True)
        # the partition alone: the triangle labels' low bits as keys
        vol.sync()
        labels = lab.download((nt,), np.uint32)
        order, offs, keys = DeviceBuffer(nt * 4 + 16), DeviceBuffer((nr.value + 2) * 4 + (1 << 18)), DeviceBuffer(nt * 4 + 16)
        res["partition"] = []
        for bits in (8, 16, 32):
            k = labels & np.uint32((1 << bits) - 1) if bits < 32 else labels
            nkeys = int(k.max()) + 1
            keys.upload(k)
            us = timed(vol, "part", lambda: L.check(lib.ivx_dev_partition_u32(keys.ptr, c64(nt), ctypes.c_uint32(nkeys), order.ptr, offs.ptr,
                                                                              vol.stream)))
            res["partition"].append({"key_bits": bits, "nkeys": nkeys, "passes": max(1, -(-max(nkeys - 1, 1).bit_length() // 8)), "us": us})
            print(json.dumps(res["partition"][-1]), flush=True)
        for b in (order, offs, keys, lab):
            b.close()
        # the split: sizes, then the filling call into buffers that exist
        nvu, nparts = ctypes.c_int64(0), ctypes.c_int64(0)
        args = (mesh.verts.ptr, c64(nv), mesh.faces.ptr, c64(nt))
        res["split_sizes_us"] = timed(vol, "sizes", lambda: L.check(lib.ivx_dev_mesh_split(
            *args, None, c64(0), None, c64(0), None, c64(0), ctypes.byref(nvu), ctypes.byref(nparts), vol.stream)))
        tb = DeviceBuffer(nparts.value * 32 + 16)
        res["split_fill_us"] = timed(vol, "fill", lambda: L.check(lib.ivx_dev_mesh_split(
            *args, ov.ptr, c64(nv), of.ptr, c64(nt), tb.ptr, c64(nparts.value), ctypes.byref(nvu), ctypes.byref(nparts), vol.stream)))
        res["used_vertices"] = nvu.value
        res["split_resident_us"] = timed(vol, "split", lambda: mesh.split().close())  # both calls + buffers, as DeviceMesh.split
        res["split_resident_wall_us"] = wall(lambda: (mesh.split().close(), vol.sync()))
        print(json.dumps({k: v for k, v in res.items() if k.startswith("split")}), flush=True)
        # per-part mass over the grouped mesh, for the bound between the wave-per-part kernel and the two-kernel path
        vol.sync()
        table = tb.download((nparts.value, 4), np.int64)
        res["part_triangles"] = {"max": int(table[:, 1].max()), "median": float(np.median(table[:, 1])),
                                 "over_1024": int(np.count_nonzero(table[:, 1] > 1024))}
        mass = DeviceBuffer(nparts.value * 64 + 16)
        res["parts_mass"] = []
        for small_max in SMALL_MAX:
            us = timed(vol, "pmass", lambda: L.check(lib.ivx_dev_mesh_parts_mass(ov.ptr, of.ptr, tb.ptr, c64(nparts.value), c64(nt),
                                                                                 c64(small_max), mass.ptr, vol.stream)))
            res["parts_mass"].append({"small_max": small_max, "us": us, "parts_over": int(np.count_nonzero(table[:, 1] > small_max))})
            print(json.dumps(res["parts_mass"][-1]), flush=True)
        one = DeviceBuffer(64)
        res["mass_whole_mesh_us"] = timed(vol, "mass", lambda: L.check(lib.ivx_dev_mesh_mass_properties(mesh.verts.ptr, mesh.faces.ptr, c64(nt),
                                                                                                       one.ptr, vol.stream)))
        for b in (mass, one, tb):
            b.close()
        # seeded select: the dominant region and two small ones; the nearest point
        vol.sync()
        big = int(np.argmax(table[:, 1]))
        faces = mesh.faces.download((nt, 3), np.int32)
        seeds = np.array([faces[np.flatnonzero(labels == r)[0], 0] for r in (big, 1, nparts.value - 1)], np.int32)
        sbuf = DeviceBuffer(64)
        sbuf.upload(seeds)
        res["select_seeded_us"] = timed(vol, "seeded", lambda: L.check(lib.ivx_dev_mesh_select_seeded(
            *args, sbuf.ptr, c64(len(seeds)), ov.ptr, c64(nv), of.ptr, c64(nt), ctypes.byref(n1), ctypes.byref(n2), vol.stream)))
        res["seeded_triangles"] = n2.value
        q = (ctypes.c_double * 3)(*[float(x) for x in np.asarray(mesh.bounds()).reshape(3, 2).mean(1)])
        res["nearest_point_us"] = timed(vol, "near", lambda: L.check(lib.ivx_dev_mesh_nearest_point(mesh.verts.ptr, c64(nv), q, sbuf.ptr, vol.stream)))
        for b in (sbuf, ov, of):
            b.close()
        verts, faces = mesh.download()
    res["host_region_labels_wall_us"] = wall(lambda: sp.region_labels(verts, faces))
    res["host_split_arrays_wall_us"] = wall(lambda: pu.split_arrays(verts, faces))
    gv, gf, tbl = pu.split_arrays(verts, faces)
    res["host_parts_mass_wall_us"] = wall(lambda: pu.parts_mass_properties(gv, gf, tbl))
    res["host_join_seeds_wall_us"] = wall(lambda: pu.JoinSeedsParts(verts, faces, seeds))
    res["host_keep_largest_wall_us"] = wall(lambda: sp.keep_largest(verts, faces))
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
