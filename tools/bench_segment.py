"""Benchmark of the U-Net segmentation (segment.py / k_unet.hip): synthetic weights in the reference's key names, a
synthetic CT-like volume.

    python tools/bench_segment.py [--out profiles/bench_segment_256.json] [--no-512] [--no-cpu]

Reports: 256^3 at overlap 0 (216 patches) and 50 (1000 patches), device-resident (DeviceVolume.segment_unet3d) and as
the host call (segment_unet3d, PCIe both ways); per-layer HIP-event times of one forward of 32 patches of 48^3 with
TF/s against the f32 MFMA peak (157.3 TF); the re-threshold of a 512^3 map (one slider move); 512^3 at overlap 50
(9261 patches); and a CPU baseline: torch's float32 forward of a few 48^3 patches in a subprocess on the CPU,
extrapolated to the patch counts (labelled as such).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TF = 157.3
LAYER_NAMES = ([n for l in range(1, 5) for n in ("enc%d_conv1" % l, "enc%d_conv2" % l, "pool%d" % l)]
               + ["bottleneck_conv1", "bottleneck_conv2"]
               + [n for l in (4, 3, 2, 1) for n in ("upconv%d" % l, "dec%d_conv1" % l, "dec%d_conv2" % l)] + ["head"])


def layer_flops(P):
    """multiply-adds x 2 per patch of each of the 27 launches (pool / head: 0 / 2 x 8 per voxel)"""
    f = (8, 16, 32, 64, 128)
    out, cin = [], 1
    for l in range(4):
        v = (P >> l) ** 3
        out += [2 * v * f[l] * cin * 125, 2 * v * f[l] * f[l] * 125, 0]
        cin = f[l]
    v = (P >> 4) ** 3
    out += [2 * v * 128 * 64 * 125, 2 * v * 128 * 128 * 125]
    for l in (3, 2, 1, 0):
        v = (P >> l) ** 3
        out += [2 * v * f[l] * f[l + 1] * 8, 2 * v * f[l] * 2 * f[l] * 125, 2 * v * f[l] * f[l] * 125]
    out.append(2 * P ** 3 * 8)
    return out


CPU_CODE = r"""
import json, sys, time, numpy as np, torch
import torch.nn as nn
torch.set_num_threads(int(sys.argv[1]))
def block(ci, f):
    return nn.Sequential(nn.Conv3d(ci, f, 5, padding=2), nn.BatchNorm3d(f), nn.ReLU(),
                         nn.Conv3d(f, f, 5, padding=2), nn.BatchNorm3d(f), nn.ReLU())
class U(nn.Module):  # the reference's Unet3D (model.py), restated for timing only
    def __init__(s):
        super().__init__()
        f = [8, 16, 32, 64, 128]
        s.e = nn.ModuleList([block(1, 8), block(8, 16), block(16, 32), block(32, 64)])
        s.b = block(64, 128)
        s.u = nn.ModuleList([nn.ConvTranspose3d(f[l + 1], f[l], 4, 2, 1) for l in range(4)])
        s.d = nn.ModuleList([block(2 * f[l], f[l]) for l in range(4)])
        s.c = nn.Conv3d(8, 1, 1)
    def forward(s, x):
        sk = []
        for e in s.e:
            x = e(x); sk.append(x); x = nn.functional.max_pool3d(x, 2)
        x = s.b(x)
        for l in (3, 2, 1, 0):
            x = s.d[l](torch.cat((s.u[l](x), sk[l]), 1))
        return torch.sigmoid(s.c(x))
m = U().eval()
x = torch.rand(1, 1, 48, 48, 48)
n = int(sys.argv[2])
with torch.no_grad():
    m(x)
    t = time.perf_counter()
    for _ in range(n):
        m(x)
    dt = (time.perf_counter() - t) / n
print(json.dumps({"s_per_patch": dt, "threads": torch.get_num_threads(), "patches_timed": n, "torch": torch.__version__}))
"""


def cpu_baseline(threads, n):
    r = subprocess.run([sys.executable, "-c", CPU_CODE, str(threads), str(n)], capture_output=True, text=True, timeout=1800)
    if r.returncode != 0:
        return {"error": r.stderr[-500:]}
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_segment_256.json"))
    ap.add_argument("--no-512", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--batch", type=int, default=None)
    args = ap.parse_args()

    import _unet_ref as R
    from invesalius3_amd import _lib as L
    from invesalius3_amd import segment as sg
    from invesalius3_amd.device import DeviceBuffer, DeviceVolume

    L.require_device()
    res = {"device": L.device_name(), "peak_tf_f32": PEAK_TF, "batch": args.batch or sg.DEFAULT_BATCH}
    net = sg.Unet3D(R.make_weights())
    kw = {} if args.batch is None else {"batch": args.batch}

    # per-layer times: one forward of 32 patches of 48^3
    P, nb = 48, 32
    x = np.random.default_rng(0).random((nb, P, P, P), dtype=np.float32)
    ws = DeviceBuffer(net.workspace_bytes(P, nb))
    din, dout = DeviceBuffer(x.nbytes), DeviceBuffer(x.nbytes)
    din.upload(x)
    ms = (ctypes.c_float * 27)()
    lib = L.lib()
    for _ in range(2):  # the first one warms up
        L.check(lib.ivx_unet3d_layer_times(net.handle, din.ptr, ctypes.c_int64(nb), P, dout.ptr, ws.ptr,
                                           ctypes.c_size_t(ws.nbytes), None, ms), "layer_times")
    fl = layer_flops(P)
    layers = []
    for name, t, f in zip(LAYER_NAMES, ms, fl):
        layers.append({"layer": name, "ms": round(t, 4), "gflop": round(f * nb / 1e9, 3),
                       "tf_s": round(f * nb / (t * 1e-3) / 1e12, 2) if f and t > 0 else None})
    tot_ms, tot_f = float(sum(ms)), float(sum(fl)) * nb
    res["forward_48_b32"] = {"ms": round(tot_ms, 3), "gflop_per_patch": round(sum(fl) / 1e9, 3),
                             "tf_s": round(tot_f / (tot_ms * 1e-3) / 1e12, 2),
                             "fraction_of_peak": round(tot_f / (tot_ms * 1e-3) / 1e12 / PEAK_TF, 3), "layers": layers}
    for b in (ws, din, dout):
        b.close()
    print(json.dumps(res["forward_48_b32"]), flush=True)

    img256 = R.ct_volume((256, 256, 256), 1)

    def run_volume(n, overlaps, host=True):
        img = np.tile(img256, (n // 256,) * 3)
        out = {}
        with DeviceVolume(img) as vol:
            for ov in overlaps:
                ncut = len(sg.patch_cuts(img.shape, 48, ov))
                vol.segment_unet3d(net, overlap=ov, **kw)  # warm-up
                t = time.perf_counter()
                vol.segment_unet3d(net, overlap=ov, **kw)
                dev_s = time.perf_counter() - t
                rec = {"patches": ncut, "tflop": round(ncut * sum(fl) / 1e12, 2), "device_resident_s": round(dev_s, 4),
                       "tf_s": round(ncut * sum(fl) / dev_s / 1e12, 2)}
                if host:
                    t = time.perf_counter()
                    sg.segment_unet3d(img, net, ov, **kw)
                    rec["host_call_s"] = round(time.perf_counter() - t, 4)
                out["overlap_%d" % ov] = rec
                print(n, ov, json.dumps(rec), flush=True)
        return out

    res["volume_256"] = run_volume(256, (0, 50))

    # one slider move at 512^3
    n = 512
    with DeviceVolume(shape=(n, n, n)) as vol:
        vol.prob = DeviceBuffer(n ** 3 * 4)
        vol.prob.upload(np.random.default_rng(2).random((n, n, n), dtype=np.float32))
        for _ in range(3):
            vol.apply_segment_threshold(0.75)
        vol.sync()
        vol.timer.collect()
        for _ in range(20):
            with vol.timer.span("thr"):
                vol.apply_segment_threshold(0.75)
        t = vol.timer.collect()["thr"]
        res["rethreshold_512"] = {"ms_median": round(float(np.median(t)), 4), "ms_min": round(float(min(t)), 4),
                                  "gb_s": round((n ** 3 * 5) / (float(np.median(t)) * 1e-3) / 1e9, 1)}
    print(json.dumps(res["rethreshold_512"]), flush=True)

    if not args.no_512:
        res["volume_512"] = run_volume(512, (50,), host=False)

    if not args.no_cpu:
        cpu = cpu_baseline(16, 3)
        if "s_per_patch" in cpu:
            cpu["extrapolated"] = True
            cpu["note"] = "torch float32 forward on the CPU, timed on 3 patches of 48^3 and multiplied by the patch count"
            cpu["est_256_overlap0_s"] = round(cpu["s_per_patch"] * 216, 1)
            cpu["est_256_overlap50_s"] = round(cpu["s_per_patch"] * 1000, 1)
            cpu["est_512_overlap50_s"] = round(cpu["s_per_patch"] * 9261, 1)
        res["cpu_baseline"] = cpu
        print(json.dumps(cpu), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
