"""Times of the geodesic measure (k_meshgeo.hip) on the bench surface: synth_v512 thresholded at (226, 3071), its
indexed mesh resident in HBM, the largest connected part of it (picks on different debris are unreachable).  Reported in
milliseconds of wall clock around the call and a stream synchronisation -- the host's looks at the device are part of the cost:
the graph build, the whole distance field from one source, point to point with stop_at for a near, a half-way and a far end (read
off that field at 5 %, 50 % and 100 % of its largest distance), and on the half-way pair a sweep of delta over {+inf, 4, 16, 64,
256} x the mean edge length and of rounds_per_look over {1, 4, 16, 64}; per run the rounds, relaxations per point and threshold
advances.  Beside them scipy.sparse.csgraph.dijkstra on one core of the same box over the same graph (the CSR the GPU built, with
the weights of include/ivx.h computed in numpy); its distances are compared with the GPU's under np.array_equal, which makes this
a full-size parity check as well.  One warm-up, median of 5.
python tools/bench_geodesic.py [n] [--out profiles/bench_geodesic_512.json]"""
import ctypes
import json
import math
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

WARM, REPS = 1, 5
SPACING = (0.5, 0.5, 0.5)
THRESHOLD = (226, 3071)
DELTAS = (math.inf, 4.0, 16.0, 64.0, 256.0)  # x mean edge length
LOOKS = (1, 4, 16, 64)


def timed(mesh, fn):
    out = []
    for _ in range(WARM + REPS):
        mesh.sync()
        t = time.perf_counter()
        fn()
        mesh.sync()
        out.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(out[WARM:]), 3)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 512
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/bench_geodesic_%d.json" % n
    img = np.ascontiguousarray(synth_v512((n, n, n)))
    lib = L.lib()
    res = {"volume": [n, n, n], "spacing": list(SPACING), "threshold": list(THRESHOLD), "device": L.device_name(), "warmup": WARM,
           "reps": REPS, "unit": "ms, wall clock around the call and a stream synchronisation, median"}
    with DeviceVolume(img, spacing=SPACING) as vol:
        vol.threshold(*THRESHOLD)
        whole = pu.DeviceMesh.from_volume(vol, vol.marching_cubes_indexed(from_binary=True, fill_border_holes=True))
        res["surface"] = {"vertices": whole.nverts, "triangles": whole.ntris}
        mesh = whole.keep_largest()
        nv, nt = mesh.nverts, mesh.ntris
        res["vertices"], res["triangles"] = nv, nt
        # the graph
        nbytes = ctypes.c_size_t(0)
        L.check(lib.ivx_mesh_graph_bytes(c64(nv), c64(nt), ctypes.byref(nbytes)))
        gbuf = DeviceBuffer(nbytes.value)
        res["graph_bytes"] = nbytes.value
        res["graph_build_ms"] = timed(mesh, lambda: L.check(lib.ivx_dev_mesh_graph_build(mesh.faces.ptr, c64(nv), c64(nt), gbuf.ptr,
                                                                                        ctypes.c_size_t(nbytes.value), mesh.stream)))
        gbuf.close()
        off, adj = mesh.graph_arrays()
        graph = mesh.graph()
        verts = mesh.verts.download((nv, 3), np.float32)
        rows = np.repeat(np.arange(nv, dtype=np.int64), np.diff(off.astype(np.int64)))
        p = verts.astype(np.float64)
        d = p[adj] - p[rows]
        w = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        del d, p
        mean_edge = float(w.mean())
        res["graph"] = {"stored_neighbours": int(len(adj)), "max_valence": int(np.diff(off.astype(np.int64)).max()),
                        "mean_edge_length": mean_edge, "zero_length_edges": int(np.count_nonzero(w == 0.0)) // 2}
        print(json.dumps({k: res[k] for k in ("vertices", "triangles", "graph_build_ms", "graph")}), flush=True)
        dist, pred = DeviceBuffer(nv * 8 + 16), DeviceBuffer(nv * 4 + 16)
        stats = (ctypes.c_int64 * 4)()

        def run(source, stop, delta, looks):
            L.check(lib.ivx_dev_mesh_geodesic_distances(mesh.verts.ptr, c64(nv), graph.ptr, c64(source), c64(stop), ctypes.c_double(delta),
                                                        ctypes.c_int(looks), dist.ptr, pred.ptr, stats, mesh.stream))

        def row(source, stop, delta_mult, looks):
            delta = 0.0 if delta_mult is None else (math.inf if math.isinf(delta_mult) else delta_mult * mean_edge)
            ms = timed(mesh, lambda: run(source, stop, delta, looks))
            return {"delta_x_mean_edge": "default" if delta_mult is None else ("inf" if math.isinf(delta_mult) else delta_mult),
                    "rounds_per_look": looks if looks > 0 else "default", "ms": ms, "rounds": int(stats[0]),
                    "relaxations_per_point": round(stats[1] / nv, 3), "threshold_advances": int(stats[2]), "host_looks": int(stats[3])}

        source = mesh.nearest_point([b for b in np.asarray(mesh.bounds()).reshape(3, 2)[:, 0]])
        res["source"] = source
        res["whole_field"] = row(source, -1, None, 0)
        mesh.sync()
        field = dist.download((nv,), np.float64)
        print(json.dumps(res["whole_field"]), flush=True)
        # scipy on one core over the same graph; its distances are the parity check
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import dijkstra
        m = csr_matrix((w, adj.astype(np.int32), off.astype(np.int32)), shape=(nv, nv))
        t = time.perf_counter()
        ref = dijkstra(m, directed=True, indices=source)
        res["scipy_dijkstra"] = {"ms": round((time.perf_counter() - t) * 1e3, 1), "threads": 1,
                                 "distances_array_equal_gpu": bool(np.array_equal(ref, field)),
                                 "points_that_differ": int(np.count_nonzero(ref != field)), "unreached": int(np.isinf(ref).sum())}
        print(json.dumps(res["scipy_dijkstra"]), flush=True)
        del m
        # near / half / far ends off that field
        fin = np.where(np.isfinite(field), field, -1.0)
        far = int(np.argmax(fin))
        ends = {"near": int(np.argmin(np.abs(fin - 0.05 * fin[far]))), "half": int(np.argmin(np.abs(fin - 0.5 * fin[far]))), "far": far}
        res["point_to_point"] = {}
        for name, end in ends.items():
            r = row(source, end, None, 0)
            mesh.sync()
            r.update({"end": end, "length_mm": float(dist.download((nv,), np.float64)[end]), "length_equals_field": None})
            r["length_equals_field"] = bool(r["length_mm"] == field[end])
            res["point_to_point"][name] = r
            print(json.dumps({name: r}), flush=True)
        res["sweep_half_pair"] = []
        for dm in DELTAS:
            for looks in LOOKS:
                res["sweep_half_pair"].append(row(source, ends["half"], dm, looks))
                print(json.dumps(res["sweep_half_pair"][-1]), flush=True)
        best = min(res["sweep_half_pair"], key=lambda r: r["ms"])
        res["chosen_defaults"] = {"delta_x_mean_edge": best["delta_x_mean_edge"], "rounds_per_look": best["rounds_per_look"],
                                  "ms": best["ms"]}
        res["sweep_whole_field"] = [row(source, -1, dm, 16) for dm in DELTAS]
        # the path call as the measure makes it (two picks: distances with stop_at, back-trace, ids and lengths to the host)
        ids = np.array([source, ends["half"]], np.int32)
        path = DeviceBuffer(nv * 4 + 16)
        seg_n, seg_len = (ctypes.c_int64 * 1)(), (ctypes.c_double * 1)()
        res["path_half_pair_ms"] = timed(mesh, lambda: L.check(lib.ivx_dev_mesh_geodesic_path(
            mesh.verts.ptr, c64(nv), graph.ptr, L.ptr(ids), c64(2), path.ptr, c64(nv), seg_n, seg_len, stats, mesh.stream)))
        res["path_half_pair"] = {"points": int(seg_n[0]), "length_mm": float(seg_len[0]), "length_equals_field": bool(seg_len[0] == field[ends["half"]])}
        for b in (dist, pred, path):
            b.close()
        mesh.close()
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
