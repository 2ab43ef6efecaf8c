#!/usr/bin/env python3
"""The mask edit history on the bound bench matrices, three ways in one run:

  (a) history    history.snapshot / EditionHistory on the bound matrix: snapshots in HBM, undo restores the mirror in place and
                 downloads the planes that changed
  (b) reference  what a caller that follows invesalius/data/mask.py pays on the host: two matrix.copy() and two np.save for
                 the save; np.load, ``mvolume[:] = array`` and Resident.touch() for the undo (the upload then rides on the
                 next use)
  (c) copy       a raw ivx_memcpy_d2d of the n bytes, the yardstick for what the codec costs beyond a copy

for *save a VOLUME pair* and for *undo + next use* (the next slice_.get_slices picture).  The matrices: the 512^3 bench image,
its 513^3 mask thresholded at (226, 3071), then one 26-connected region growth from the brightest voxel; undo and redo walk
between the two states.  Wall clock around the Python calls (they end synchronised), median of five after a warm-up.  Also
recorded: the encoded bytes over n of both masks, the planes an undo downloads, the bytes the copy helpers moved, the three
device passes alone, and the byte model of DESIGN 7m over the copy rate this very run measured.

    python tools/bench_history.py               # 512^3 image, 513^3 mask
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

p = argparse.ArgumentParser()
p.add_argument("--size", type=int, default=512)
p.add_argument("--reps", type=int, default=5)
args = p.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import BONE, synth_v512  # noqa: E402
from invesalius3_amd import _lib as L  # noqa: E402
from invesalius3_amd import history, resident, slice_, styles  # noqa: E402
from invesalius3_amd import mask as mask_mod  # noqa: E402
from invesalius3_amd import slice_display as D  # noqa: E402
from invesalius3_amd.device import DeviceBuffer  # noqa: E402


def timeit(fn, before=None):
    t, moved = [], None
    for i in range(args.reps + 1):
        if before is not None:
            before(i)
        c0 = resident.transfer_stats()
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i:
            t.append(dt)
            moved = {k: v - c0[k] for k, v in resident.transfer_stats().items()}
    return {"ms": round(float(np.median(t)) * 1e3, 3), "min_ms": round(min(t) * 1e3, 3), "max_ms": round(max(t) * 1e3, 3), "calls": len(t),
            "moved_per_call": moved}


def main():
    n = args.size
    L.require_device()
    img = synth_v512((n, n, n))
    mask = np.zeros((n + 1,) * 3, np.uint8)
    slice_.do_threshold_to_all_slices(mask, img, BONE)
    for ax in range(3):  # every slice of every orientation up to date, as after the viewer has shown them
        idx = [slice(0, 1)] * 3
        idx[ax] = slice(1, None)
        mask[tuple(idx)] = 1
    nbytes = mask.nbytes
    z, y, x = (int(v) for v in np.unravel_index(int(np.argmax(img)), img.shape))
    st = D.DisplayState(window_width=2000.0, window_level=300.0)
    st.set_colour_table("Default ")
    image_range = (img.min(), img.max())
    res = {}
    bound = [slice_.bind_image(img), mask_mod.bind_matrix(mask)]
    rm = bound[1]
    thresholded = history.snapshot(mask)
    styles.do_3d_seg(img, mask, (x, y, z), method="threshold", con_3d=26, t0=BONE[0], t1=BONE[1])
    grown = history.snapshot(mask)  # (the tool's numpy write goes up here)
    res["encoded_bytes_over_n"] = {"thresholded": round(thresholded.device_bytes / nbytes, 4), "grown": round(grown.device_bytes / nbytes, 4)}
    res["literal_blocks"] = {"thresholded": thresholded.literal_blocks, "grown": grown.literal_blocks, "blocks": -(-nbytes // 64)}

    def picture():
        slice_.get_slices(img, mask, "AXIAL", n // 2, 1, st, image_range=image_range)

    # ---- save a VOLUME pair -------------------------------------------------------------------------------------------
    h = history.EditionHistory()
    save = res.setdefault("save a VOLUME pair", {})
    save["history"] = timeit(lambda: h.new_node(0, "VOLUME", history.snapshot(mask), history.snapshot(mask), False), lambda i: h.clear_history())
    h.clear_history()
    tmp = tempfile.mkdtemp()
    f1, f2 = os.path.join(tmp, "a.npy"), os.path.join(tmp, "b.npy")

    def reference_save():
        a, b = mask.copy(), mask.copy()
        np.save(f1, a)
        np.save(f2, b)

    save["reference"] = timeit(reference_save)
    d_src, d_dst = DeviceBuffer(nbytes), DeviceBuffer(nbytes)
    d_src.upload(mask)

    def raw_copy(times):
        for _ in range(times):
            L.check(L.lib().ivx_memcpy_d2d(d_dst.ptr, d_src.ptr, ctypes.c_size_t(nbytes), None))
        L.synchronize()

    save["copy"] = timeit(lambda: raw_copy(2))
    # ---- undo + next use ----------------------------------------------------------------------------------------------
    h.new_node(0, "VOLUME", grown, thresholded, False)
    planes = []

    def step():
        s0 = resident.transfer_stats()["d2h_bytes"]
        (h.undo if h.index == 1 else h.redo)(mask, None)
        planes.append((resident.transfer_stats()["d2h_bytes"] - s0) // ((n + 1) * (n + 1)))
        picture()

    picture()
    undo = res.setdefault("undo + next use", {})
    undo["history"] = timeit(step)
    undo["planes_downloaded"] = planes[-1]
    undo["planes"] = n + 1
    if h.index == 0:
        h.redo(mask, None)
    np.save(f1, mask)  # (the grown state; the host copy equals the mirror here)
    saved_grown = mask.copy()

    def reference_undo():
        arr = np.load(f1)
        mask[:] = arr
        rm.touch()
        picture()

    undo["reference"] = timeit(reference_undo)
    assert np.array_equal(mask, saved_grown)
    undo["copy"] = timeit(lambda: raw_copy(1))
    # ---- the three device passes alone, against the byte model over the measured copy rate -----------------------------
    rate = 2 * nbytes / (undo["copy"]["ms"] * 1e-3)  # a copy reads n and writes n
    hb, lit = history.header_bytes(nbytes), grown.literal_blocks
    hdr, pool, nlit = DeviceBuffer(hb), DeviceBuffer(max(64 * lit, 16)), L.c_i64(0)
    lib = L.lib()

    def scan():
        L.check(lib.ivx_dev_mask_snapshot_scan(d_src.ptr, nbytes, hdr.ptr, ctypes.byref(nlit), None))

    def pack():
        L.check(lib.ivx_dev_mask_snapshot_pack(d_src.ptr, nbytes, hdr.ptr, pool.ptr, lit, None))
        L.synchronize()

    d_src.upload(mask)
    passes = res.setdefault("device passes (grown mask)", {"copy_rate_GBps": round(rate / 1e9, 1)})
    for name, fn, model in (("scan", scan, nbytes + hb), ("pack", pack, 2 * 64 * lit + hb)):
        e = passes[name] = timeit(fn)
        e["model_bytes"], e["model_ms"] = model, round(model / rate * 1e3, 3)
        e["measured / model"] = round(e["ms"] / max(e["model_ms"], 1e-6), 2)
    assert nlit.value == lit
    flags = DeviceBuffer(n + 1)

    def restore_onto(src_snapshot):
        def run():
            L.check(lib.ivx_dev_mask_snapshot_restore(d_dst.ptr, nbytes, src_snapshot.header.ptr, src_snapshot.pool.ptr,
                                                      src_snapshot.literal_blocks, (n + 1) * (n + 1), flags.ptr, None))
            L.synchronize()
        return run

    raw_copy(1)  # d_dst = the grown mask
    e = passes["restore onto identical bytes"] = timeit(restore_onto(grown))
    e["model_bytes"] = nbytes + hb + 64 * lit
    state = {"i": 0}

    def alternate():
        s = (thresholded, grown)[state["i"] & 1]
        state["i"] += 1
        restore_onto(s)()

    e = passes["restore, the growth's planes differ"] = timeit(alternate)
    e["model_bytes"] = nbytes + hb + 64 * lit + planes[-1] * (n + 1) * (n + 1)
    for k in ("restore onto identical bytes", "restore, the growth's planes differ"):
        e = passes[k]
        e["model_ms"] = round(e["model_bytes"] / rate * 1e3, 3)
        e["measured / model"] = round(e["ms"] / max(e["model_ms"], 1e-6), 2)
    h.clear_history()
    # ---- tool -> undo -> redo -> tool on the bound matrix: what each step moves ------------------------------------------
    seq = res.setdefault("crop -> undo -> redo -> crop, bytes moved", {})
    q = n // 4

    def counted(name, fn):
        c0 = resident.transfer_stats()
        t0 = time.perf_counter()
        fn()
        seq[name] = dict({k: v - c0[k] for k, v in resident.transfer_stats().items()}, ms=round((time.perf_counter() - t0) * 1e3, 3))

    def crop(lim):
        with history.recorded(h, mask):
            styles.crop_mask(mask, None, lim)

    counted("crop (recorded)", lambda: crop((q, 3 * q, q, 3 * q, q, 3 * q)))
    counted("undo", lambda: h.undo(mask, None))
    counted("redo", lambda: h.redo(mask, None))
    counted("crop again (recorded)", lambda: crop((q + 8, 3 * q - 8, q, 3 * q, q, 3 * q)))
    seq["note"] = "crop_mask itself writes the whole matrix back to the host (DESIGN 7i); the history adds nothing to it"
    h.undo(mask, None)
    h.undo(mask, None)
    h.undo(mask, None)
    assert np.array_equal(mask, saved_grown)
    h.clear_history()
    for b in (d_src, d_dst, hdr, pool, flags):
        b.close()
    for r in bound:
        r.release()
    for f in (f1, f2):
        if os.path.exists(f):
            os.remove(f)
    os.rmdir(tmp)
    print(json.dumps({"size": "%d^3 image, %d^3 mask (%d bytes)" % (n, n + 1, nbytes), "device": L.device_name(),
                      "protocol": "wall clock around the Python calls, synchronised inside the timed span, median of %d after one warm-up "
                                  "(min / max beside it); moved_per_call: bytes the library's copy helpers moved; model: the byte model "
                                  "of DESIGN 7m over the device-to-device copy rate measured in this run" % args.reps,
                      "results": res}, indent=1))


if __name__ == "__main__":
    main()
