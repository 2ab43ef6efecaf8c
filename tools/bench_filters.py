"""Device times of the image filters (k_filter.hip) on the resident synth_v512 volume (HIP events, 2 warm-ups, median of
five), with the algorithmic bytes, the bound (HBM copy rate, or the float64 rate without FMA for the wide Gaussians),
the share of that bound, and the host-level call (pageable numpy in and out over PCIe).  scipy on one core at 256^3 is
the CPU baseline the reference runs (filters.py:5-66).
python tools/bench_filters.py [n] [--no-scipy | --scipy-only]   (--scipy-only: the CPU baseline alone, no device needed)"""
import ctypes
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from bench import synth_v512  # noqa: E402
from invesalius3_amd import _lib as L  # noqa: E402
from invesalius3_amd import filters as F  # noqa: E402
from invesalius3_amd.device import DeviceBuffer, DeviceVolume  # noqa: E402

HBM_COPY_GBS = 6290.0    # measured device copy rate (profiles / DESIGN.md)
F64_NOFMA_TOPS = 39.3    # MI355X vector f64 78.6 TFLOP/s counts an FMA as two: one unfused op per cycle-lane is half

# (name, filter_type, value, plane_axis)
CASES = [("gaussian_s1", 0, 1.0, -1), ("gaussian_s10", 0, 10.0, -1), ("mean_7", 2, 3.0, -1), ("mean_31", 2, 15.0, -1),
         ("median_3", 1, 1.0, -1), ("median_5", 1, 3.0, -1), ("sharpen_v1", 3, 1.0, -1), ("border_s1", 5, 1.0, -1),
         ("gaussian_s1_2d_axial", 0, 1.0, 0), ("median_5_2d_axial", 1, 3.0, 0), ("median_5_2d_sagittal", 1, 3.0, 2),
         ("mean_31_2d_coronal", 2, 15.0, 1), ("border_s1_2d_axial", 5, 1.0, 0)]


def floor_of(ft, v, plane, n):
    """(bytes moved by the algorithm, bound name, floor in ms)"""
    passes = 3 if plane < 0 else 2
    if ft in (0, 4):
        _w, r = F.gaussian_weights(v)
        nbytes = passes * 4 * n
        ops = passes * n * (3 * r + 1)  # per tap pair: add, mul, add; plus the centre product
    elif ft == 2:
        nbytes, ops = passes * 4 * n, 0
    elif ft == 1:
        nbytes, ops = 4 * n, 0
    elif ft == 3:
        nbytes, ops = (2 + 8) * n + (passes - 1) * 16 * n + (2 + 8 + 2) * n, passes * n * 13
        # int16 -> f64, f64 -> f64 passes, min/max read, final read of m and b, write
    else:
        nbytes = (2 + 8) * n + (passes - 1) * 16 * n + 16 * n + 2 * n + 8 * n + 10 * n
        ops = passes * n * 13
    hbm = nbytes / (HBM_COPY_GBS * 1e6)
    f64 = ops / (F64_NOFMA_TOPS * 1e9)
    return nbytes, ("f64" if f64 > hbm else "HBM"), max(hbm, f64)


def scipy_baseline():
    """the reference's filters on one core (scipy.ndimage is single-threaded) at 256^3, seconds"""
    import scipy.ndimage as ndi
    small = synth_v512((256, 256, 256))
    ref = {"gaussian_s1": lambda m: ndi.gaussian_filter(m, 1.0), "gaussian_s3": lambda m: ndi.gaussian_filter(m, 3.0),
           "mean_7": lambda m: ndi.uniform_filter(m, 7), "median_3": lambda m: ndi.median_filter(m, 3),
           "median_5": lambda m: ndi.median_filter(m, 5)}
    res = {}
    for name, fn in ref.items():
        t0 = time.perf_counter()
        fn(small)
        res[name + "_s"] = round(time.perf_counter() - t0, 2)
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 512
    if "--scipy-only" in sys.argv:
        print(json.dumps({"scipy_1core_256": scipy_baseline()}))
        return
    img = synth_v512((n, n, n))
    N = img.size
    vol = DeviceVolume(img)
    lib = L.lib()
    out = {"n": n, "device": L.device_name(), "filters": {}}
    shape = L.i64(img.shape)
    res = DeviceBuffer(N * 2)
    nb = ctypes.c_size_t(0)
    L.check(lib.ivx_filter_scratch_bytes(F.BORDER, shape, -1, ctypes.byref(nb)))  # the largest of the kinds
    scratch = DeviceBuffer(nb.value)

    def dev_call(ft, v, plane):
        st, src = vol.stream, vol.image.raw
        if ft == 1:
            return lib.ivx_dev_filter_median_i16(src, shape, plane, F.median_size(v), res.ptr, st)
        if ft == 2:
            return lib.ivx_dev_filter_mean_i16(src, shape, plane, F.mean_size(v), res.ptr, scratch.ptr, st)
        w, r = F.gaussian_weights(1.0 if ft == 3 else v)
        wp = L.ptr(w)
        if ft == 3:
            return lib.ivx_dev_filter_sharpen_i16(src, shape, plane, ctypes.c_double(v), wp, r, res.ptr, scratch.ptr, st)
        if ft == 5:
            return lib.ivx_dev_filter_border_i16(src, shape, plane, 1, wp, r, res.ptr, scratch.ptr, st)
        return lib.ivx_dev_filter_gaussian_i16(src, shape, plane, wp, r, res.ptr, scratch.ptr, st)

    for name, ft, v, plane in CASES:
        for _ in range(2):
            L.check(dev_call(ft, v, plane), name)
        vol.sync()
        vol.timer.collect()
        for _ in range(5):
            with vol.timer.span(name):
                L.check(dev_call(ft, v, plane), name)
        vol.sync()
        ms = float(np.median(vol.timer.collect()[name]))
        nbytes, bound, floor_ms = floor_of(ft, v, plane, N)
        rec = {"filter_type": ft, "value": v, "plane_axis": plane, "ms": round(ms, 4), "algorithmic_GB": round(nbytes / 1e9, 3),
               "algorithmic_GB_s": round(nbytes / ms / 1e6, 1), "bound": bound, "floor_ms": round(floor_ms, 4),
               "share_of_bound": round(floor_ms / ms, 3)}
        # the host-level call: numpy in, numpy out (PCIe both ways, pageable)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            F.image_filter(img, ft, v, plane)
            ts.append((time.perf_counter() - t0) * 1e3)
        rec["host_call_ms"] = round(float(np.median(ts)), 2)
        out["filters"][name] = rec
    if "--no-scipy" not in sys.argv:
        out["scipy_1core_256"] = scipy_baseline()
    vol.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
