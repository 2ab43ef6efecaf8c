"""The weld of the surface import (csrc/k_meshweld.hip) on the bench surface's soup, against the host weld the
tree had before it: one run on the GPU box, the numbers written as markdown (profiles/surface_import.md).

    python tools/probe_surface_import.py [--size 512] [--reps 5] --out FILE.md

(a) the host weld: the np.unique lines of surface_process.join_surface_pieces applied to the same soup, wall clock, once;
(b) the device weld: ivx_dev_stl_unpack and ivx_dev_mesh_weld with their inputs resident, from HIP events around each queued
    chain (median of --reps), and the end-to-end wall time from the file's bytes in host memory through
    DeviceMesh.from_stl_bytes (upload, unpack, weld, the count download), with the table size and the walk-length histogram
    the status words give."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_weld(soup):
    """surface_process.join_surface_pieces, the merge lines (raw-bit keys, first appearance order)"""
    soup = soup.reshape(-1, 3)
    key = np.ascontiguousarray(soup).view([("", np.uint32)] * 3).ravel()
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return soup[first[order]], rank[inverse].reshape(-1, 3).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()

    import bench
    from invesalius3_amd import _lib as L
    from invesalius3_amd import polydata_utils as pu
    from invesalius3_amd import surface as S
    from invesalius3_amd.device import DeviceBuffer, DeviceVolume, Timer

    L.require_device()
    n = args.size
    img = bench.synth_v512((n, n, n), seed=bench.SEED)
    vol = DeviceVolume(img, spacing=(0.5, 0.5, 0.5))
    vol.threshold(*bench.BONE)
    v, f = vol.marching_cubes_indexed(download=True)
    vol.close()
    soup = np.ascontiguousarray(v[f])
    nt = len(soup)
    del img

    t0 = time.perf_counter()
    hv, hf = host_weld(soup)
    host_ms = (time.perf_counter() - t0) * 1e3

    rec = np.zeros(nt, dtype=[("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")])
    rec["v"] = soup
    data = b"probe".ljust(80) + np.uint32(nt).tobytes() + rec.tobytes()
    del rec
    raw = np.frombuffer(data, np.uint8)

    lib = L.lib()
    nb = ctypes.c_size_t(0)
    L.check(lib.ivx_mesh_weld_bytes(ctypes.c_int64(nt), ctypes.byref(nb)))
    file_buf, soup_buf, flag = DeviceBuffer(len(raw) + 16), DeviceBuffer(nt * 36 + 16), DeviceBuffer(16)
    scratch, cnt = DeviceBuffer(nb.value + 16), DeviceBuffer(L.WELD_COUNT_WORDS * 4)
    ov, of = DeviceBuffer(nt * 36 + 16), DeviceBuffer(nt * 12 + 16)
    file_buf.upload(raw)
    flag.zero()
    timer = Timer(None)
    for _ in range(args.reps + 1):  # (the first run warms up)
        with timer.span("unpack"):
            L.check(lib.ivx_dev_stl_unpack(file_buf.ptr, ctypes.c_int64(nt), soup_buf.ptr, flag.ptr, None))
        with timer.span("weld"):
            L.check(lib.ivx_dev_mesh_weld(soup_buf.ptr, ctypes.c_int64(nt), scratch.ptr, ov.ptr, of.ptr, cnt.ptr, None))
        L.synchronize()
    ms = {k: statistics.median(x[1:]) for k, x in timer.collect().items()}
    counts = S.counts_dict(cnt.download((L.WELD_COUNT_WORDS,), np.uint32), nt)
    gv = ov.download((counts["vertices"], 3), np.float32)
    gf = of.download((counts["facets"], 3), np.int32)
    same = counts["dropped"] == 0 and np.array_equal(gf, hf) and np.array_equal(gv.view(np.uint32), hv.view(np.uint32))
    for b in (file_buf, soup_buf, flag, scratch, cnt, ov, of):
        b.close()

    e2e = []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        mesh = pu.DeviceMesh.from_stl_bytes(data)
        e2e.append((time.perf_counter() - t0) * 1e3)
        mesh.close()
    e2e_ms = statistics.median(e2e[1:])

    hist = counts["probe_histogram"]
    names = ["0", "1", "2-3", "4-7", "8-15", "16-31", "32-63", "64-127", "128-255", "256-511", "512-1023", "1024-2047", "2048-4095",
             "4096-8191", "8192-16383", ">=16384"]
    lines = ["# Surface import: the weld on the bench surface's soup", "",
             "`python tools/probe_surface_import.py --size %d --reps %d` on %s." % (n, args.reps, L.device_name()), "",
             "The soup: %d triangles (%d corners) of the %d^3 bench volume's bone surface; %d points after the weld, %d facets dropped."
             % (nt, 3 * nt, n, counts["vertices"], counts["dropped"]),
             "The device weld's vertices and faces equal the host weld's bit for bit: %s "
             "(they must where no facet is degenerate and no coordinate is a minus zero)." % ("yes" if same else "NO"), "",
             "| what | ms |", "|---|---|",
             "| (a) host weld: the `np.unique` lines of `join_surface_pieces`, wall clock, one run | %.1f |" % host_ms,
             "| (b) `ivx_dev_stl_unpack`, file bytes resident, HIP events, median of %d | %.3f |" % (args.reps, ms["unpack"]),
             "| (b) `ivx_dev_mesh_weld`, soup resident, HIP events around the queued chain, median of %d | %.3f |" % (args.reps, ms["weld"]),
             "| (b) end to end: file bytes in host memory -> `DeviceMesh.from_stl_bytes` (upload of %.0f MB, unpack, weld, counts), wall clock, median of %d | %.1f |"
             % (len(raw) / 1e6, args.reps, e2e_ms), "",
             "Table: %d slots (%.0f MB), load %.3f; longest walk %d slots past the home slot." % (counts["slots"], counts["slots"] * 4 / 1e6,
                                                                                            counts["vertices"] / counts["slots"], counts["max_probe"]), "",
             "| slots walked past the home slot | corners |", "|---|---|"]
    lines += ["| %s | %d |" % (names[q], hist[q]) for q in range(16) if hist[q]]
    lines += ["", "Host weld over end-to-end device import: %.1fx." % (host_ms / e2e_ms) if e2e_ms < host_ms else
              "The device import is NOT ahead of the host weld once the upload is counted (%.1f ms against %.1f ms)." % (e2e_ms, host_ms), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
