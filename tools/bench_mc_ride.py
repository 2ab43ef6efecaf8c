#!/usr/bin/env python3
"""The price of a count nobody uses: region-growing steps (out_mask zeros + threshold + region growing, no surface call)
behind ONE surface call, with the ride on and off (DeviceVolume._ride.enabled; invesalius3_amd/mc_ride.py).  With the ride on
the first step behind the surface call carries marching cubes' count in its mask write and the later ones do not (the ride
is disarmed until a surface call arms it again), so the first step's extra time is the whole price of a streak of clicks.

    python tools/bench_mc_ride.py [--size 512] [--reps 9]

Each figure is the wall clock of one step between two stream synchronisations, median (min .. max) of --reps; one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scipy.ndimage import generate_binary_structure  # noqa: E402

from bench import BONE, synth_v512  # noqa: E402
from invesalius3_amd.device import DeviceVolume  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()
n = args.size
img = synth_v512((n, n, n))
z, y, x = np.unravel_index(int(np.argmax(img)), img.shape)
seed, strct = (int(x), int(y), int(z)), generate_binary_structure(3, 3)
vol = DeviceVolume(img)
vol.timer.only = set()


def click():
    vol.zero_out_mask()
    vol.threshold(BONE[0], BONE[1], preserve=False)
    vol.region_grow([seed], BONE[0], BONE[1], strct, fill=1, select_value=254)


def timed_click():
    vol.sync()
    t = time.perf_counter()
    click()
    vol.sync()
    return (time.perf_counter() - t) * 1e3


def streak(ride):
    """surface call, then three clicks: -> ms of the first, second and third, and whether the first rode"""
    vol._ride.enabled = ride
    click()
    vol.marching_cubes(from_binary=True)
    before = vol._ride.rides
    ms = [timed_click() for _ in range(3)]
    return ms, vol._ride.rides - before


def stat(v):
    return {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


for _ in range(3):  # warm-up: buffers, workspaces, the steady state of the surface call
    click()
    vol.marching_cubes(from_binary=True)
res = {"size": n, "reps": args.reps}
runs = {True: [], False: []}
for _ in range(args.reps):  # ride on and off alternately
    for ride in (True, False):
        ms, rode = streak(ride)
        assert rode == int(ride), (ride, rode)
        runs[ride].append(ms)
for ride, key in ((True, "ride_on"), (False, "ride_off")):
    a = np.array(runs[ride])
    res[key] = {"first_click": stat(a[:, 0]), "second_click": stat(a[:, 1]), "third_click": stat(a[:, 2])}
res["wasted_count_ms"] = round(res["ride_on"]["first_click"]["ms"] - res["ride_off"]["first_click"]["ms"], 4)
print(json.dumps(res))
vol.close()
