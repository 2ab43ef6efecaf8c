"""Golden vectors from the REFERENCE ITSELF for the slice editing tools: Slice.edit_mask_pixel, get_mask_slice and
apply_slice_buffer_to_mask (invesalius/data/slice_.py:656-744, 1121-1175, 1925-1967), the marker brush and the generic brush
(WaterShedInteractorStyle / BaseImageEditionInteractorStyle.edit_mask_pixel, styles.py:2000-2069, 392-461),
FloodFillSegmentInteractorStyle.do_2d_seg (:3082-3149), CropMaskInteractorStyle.CropMask (:2654-2694) and the two
_calculate_area_pixels (cursor_actors.py:302-330, 377-395).  The reference's modules are imported from its checkout (INVESALIUS_REFERENCE) under the
stand-in finder and the methods called unbound on plain namespaces; the Rust flood under do_2d_seg is bound to oracle/'s pinned
restatement, as in make_golden_ref_3dseg.py.

    INVESALIUS_REFERENCE=<the reference's checkout> python3 tests/golden/make_golden_ref_editor.py

The case lists below are the fixture's inputs: they are stored next to the outputs, and the tests read them from the file.
"""
import os
import sys
import tempfile
import types
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden_ref_dowatershed as M  # noqa: E402
from oracle import oracle as O  # noqa: E402

ORIENTATIONS = ("AXIAL", "CORONAL", "SAGITAL")
SPACING = (0.5, 0.75, 2.0)
EDITION_RANGE = (100.5, 900)     # a float bound: numpy compares int16 with it, the kernel with its ceil
THRESHOLD_RANGE = (226, 3071)
# the list of the issue (a 7 x 7 disk on a 20-wide slice), the four edges and corners, windows that miss the slice, floats, and
# the flat-integer form (one number instead of a pair)
POSITIONS = [(3, 3), (2, 2), (1, 5), (0, 0), (-4, 5), (-5, 5), (-8, 5), (23, 10), (30, 10), (10, -9), (22, 10), (5.5, 5.5),
             (10, 0), (10, 1000), (0, 4), (1000, 4), (-1000, -1000), (7.99, 3.01), (-0.5, -0.5), 45, 0, 170, 10 ** 6]


def slice_of(a, orientation, n):
    return a[n] if orientation == "AXIAL" else (a[:, n, :] if orientation == "CORONAL" else a[:, :, n])


def main(path):
    tmp_root = tempfile.mkdtemp(prefix="ref_editor_")  # the reference's temporary files and its HOME: outside the tree
    tempfile.tempdir = tmp_root
    os.environ["HOME"] = tmp_root
    M._Finder.ROOTS = tuple(r for r in M._Finder.ROOTS if r != "invesalius_rs")
    native = M._Fake("invesalius_rs._native")
    native.floodfill_threshold = lambda data, seeds, t0, t1, fill, strct, out: O.floodfill_threshold(data, seeds, t0, t1, fill, strct, out)
    sys.modules["invesalius_rs._native"] = native
    sys.meta_path.insert(0, M._Finder())
    import pubsub.pub
    pubsub.pub.subscribe = lambda *a, **k: (None, True)
    pubsub.pub.sendMessage = lambda *a, **k: None
    reference = os.environ.get("INVESALIUS_REFERENCE")
    if not reference or not os.path.isdir(os.path.join(reference, "invesalius")):
        raise SystemExit("set INVESALIUS_REFERENCE to the reference's checkout (the directory that holds invesalius/)")
    sys.path.insert(0, reference)
    from invesalius.data import cursor_actors as rca
    from invesalius.data import slice_ as rs
    from invesalius.data import styles as rst
    rs.ses = mock.MagicMock()
    rs.Publisher.sendMessage = lambda *a, **k: None
    rst.Publisher.sendMessage = lambda *a, **k: None

    rng = np.random.default_rng(20261020)
    d = {"spacing": np.array(SPACING), "edition_range": np.array(EDITION_RANGE), "threshold_range": np.array(THRESHOLD_RANGE)}

    # ---- footprints -------------------------------------------------------------------------------------------------------------
    cur_names = []
    for fmt, cls in (("circle", rca.CursorCircle), ("rectangle", rca.CursorRectangle)):
        for unit in ("mm", "µm", "px"):
            for ori in ORIENTATIONS:
                for radius in (0.4, 3, 15, 30.5):
                    c = types.SimpleNamespace(radius=radius * (1000 if unit == "µm" else 1), unit=unit, orientation=ori, spacing=SPACING)
                    cls._calculate_area_pixels(c)
                    name = "cur_%s_%s_%s_%s" % (fmt, {"µm": "um"}.get(unit, unit), ori, radius)
                    cur_names.append(name)
                    d[name] = np.array(c.points)
    d["cursor_names"] = np.array(cur_names)

    def circle_px(r):
        c = types.SimpleNamespace(radius=r, unit="px", orientation="AXIAL", spacing=SPACING)
        rca.CursorCircle._calculate_area_pixels(c)
        return np.array(c.points)

    footprints = [circle_px(3), np.ones((1, 1), bool), np.ones((3, 5), bool), circle_px(30), circle_px(40)]
    assert footprints[0].shape == (7, 7) and footprints[4].shape == (81, 81)
    for k, f in enumerate(footprints):
        d["footprint_%d" % k] = f

    # ---- the volumes ------------------------------------------------------------------------------------------------------------
    def volume(shape, seed):
        img, am = M.ct_like(shape, seed)
        m = np.zeros(tuple(s + 1 for s in shape), np.uint8)
        m[1:, 1:, 1:] = rng.choice(np.array([0, 1, 2, 253, 254, 255], np.uint8), size=shape)
        for ax in range(3):  # flags mixed across 0, 1 and 2 on every axis
            idx = [0, 0, 0]
            for k in range(1, m.shape[ax]):
                idx[ax] = k
                m[tuple(idx)] = k % 3
        return img, m, am

    img, mask_in, am = volume((9, 20, 24), 91)
    big_img, big_mask_in, _ = volume((3, 100, 120), 92)
    d.update(img=img, mask_in=mask_in, big_img=big_img, big_mask_in=big_mask_in)

    # ---- Slice.edit_mask_pixel: one dab on a fresh copy of the buffer slice -----------------------------------------------------------
    raised = []

    def dab(image3, padded, ori, n, op, fp, pos):
        bs = types.SimpleNamespace(mask=np.array(slice_of(padded[1:, 1:, 1:], ori, n)), image=slice_of(image3, ori, n),
                                   discard_vtk_mask=lambda: None)
        self_ = types.SimpleNamespace(buffer_slices={ori: bs}, spacing=SPACING,
                                      current_mask=types.SimpleNamespace(edition_threshold_range=EDITION_RANGE))
        before = bs.mask.copy()
        try:
            rs.Slice.edit_mask_pixel(self_, op, footprints[fp], pos, 3, ori)
        except ValueError:
            # BRUSH_THRESH_ADD_ONLY / _ERASE_ONLY with a window that ends left of or above the slice: xf (or yf) is negative,
            # ``mask[yi:yf, xi:xf]`` counts it from the far end and ``index & (roi_i >= ...)`` cannot broadcast (slice_.py:733,
            # 735).  The GUI's event handler drops the exception; nothing was written.  Recorded as the no-op it amounts to.
            assert op in (4, 5) and np.array_equal(bs.mask, before)
            raised.append((ori, n, op, fp, pos))
        return bs.mask

    def enc(pos):
        return (float(pos[0]), float(pos[1]), 0.0) if hasattr(pos, "__iter__") else (float(pos), 0.0, 1.0)

    N = {"AXIAL": 4, "CORONAL": 7, "SAGITAL": 23}   # the sagittal one is the last column of the matrix
    for vol_name, image3, padded, plan in (
            ("small", img, mask_in, [(op, 0, POSITIONS) for op in range(6)] + [(op, fp, POSITIONS[:4] + POSITIONS[10:13] + [45])
                                                                                 for op in (0, 2, 5) for fp in (1, 2, 3)]),
            ("big", big_img, big_mask_in, [(op, 4, [(50, 50), (3, 2), (118.5, 97), 5000, (-45, 50)]) for op in (0, 3, 4)])):
        for ori in ORIENTATIONS:
            n = N[ori] if vol_name == "small" else 1
            meta, outs = [], []
            for op, fp, positions in plan:
                for pos in positions:
                    meta.append((n, op, fp) + enc(pos))
                    outs.append(dab(image3, padded, ori, n, op, fp, pos))
            d["dabs_%s_%s_meta" % (vol_name, ori)] = np.array(meta, np.float64)
            d["dabs_%s_%s_out" % (vol_name, ori)] = np.stack(outs)

    d["dabs_reference_raised"] = np.array(len(raised))
    print(len(raised), "dabs on which the reference raises instead of writing nothing")

    # ---- the marker brush and the generic fill-value brush: matrices of the image's shape -------------------------------------------
    markers_in = rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), size=img.shape)
    d["markers_in"] = markers_in
    meta, outs = [], []
    for style, value in (("ws", 1), ("ws", 2), ("base", 77)):
        for ori in ORIENTATIONS:
            for fp, pos in ((0, (3, 3)), (0, (22, 10)), (2, (0, 0)), (0, 45), (3, (10, 5)), (0, (-8, 5))):
                mat = markers_in.copy()
                self_ = types.SimpleNamespace(matrix=mat, fill_value=value, viewer=types.SimpleNamespace(slice_=types.SimpleNamespace(spacing=SPACING)))
                cls = rst.WaterShedInteractorStyle if style == "ws" else rst.BaseImageEditionInteractorStyle
                cls.edit_mask_pixel(self_, value, N[ori] - 1 if ori == "SAGITAL" else N[ori], footprints[fp], pos, 3, ori)
                meta.append((ORIENTATIONS.index(ori), N[ori] - 1 if ori == "SAGITAL" else N[ori], value, fp) + enc(pos))
                outs.append(mat)
    d["fill_meta"], d["fill_out"] = np.array(meta, np.float64), np.stack(outs)

    # ---- get_mask_slice and apply_slice_buffer_to_mask ---------------------------------------------------------------------------------
    def slice_ns(matrix, image3):
        cur = types.SimpleNamespace(matrix=matrix, threshold_range=THRESHOLD_RANGE, save_history=lambda *a, **k: None, was_edited=False)
        s = types.SimpleNamespace(matrix=image3, current_mask=cur, spacing=SPACING,
                                  buffer_slices={o: mock.MagicMock(index=-1, mask=None) for o in ORIENTATIONS})
        s.do_threshold_to_a_slice = lambda *a, **k: rs.Slice.do_threshold_to_a_slice(s, *a, **k)
        return s, cur

    meta, mats, rets = [], [], {}
    for ori in ORIENTATIONS:
        for n in (2, 3, 4):  # flags 0, 1, 2
            mat = mask_in.copy()
            s, _ = slice_ns(mat, img)
            got = rs.Slice.get_mask_slice(s, ori, n)
            meta.append((ORIENTATIONS.index(ori), n))
            mats.append(mat)
            rets["getslice_ret_%s_%d" % (ori, n)] = np.array(got)
    d["getslice_meta"], d["getslice_out"] = np.array(meta), np.stack(mats)
    d.update(rets)

    mats, prevs = [], {}
    for ori in ORIENTATIONS:
        mat = mask_in.copy()
        s, cur = slice_ns(mat, img)
        b = rng.choice(np.array([0, 1, 254, 255], np.uint8), size=slice_of(img, ori, 5).shape)
        s.buffer_slices[ori] = types.SimpleNamespace(mask=b, index=5)
        hist = []
        cur.save_history = lambda index, orientation, b_mask, p_mask, hist=hist: hist.append(np.array(p_mask))
        rs.Slice.apply_slice_buffer_to_mask(s, ori)
        d["apply_b_%s" % ori] = b
        prevs["apply_prev_%s" % ori] = hist[0]
        mats.append(mat)
    d["apply_out"] = np.stack(mats)
    d.update(prevs)

    # ---- do_2d_seg ----------------------------------------------------------------------------------------------------------------------
    seed = (int(am[2]), int(am[1]), int(am[0]))  # (x, y, z) of the brightest voxel
    cases = [("threshold", False, 4, "AXIAL", dict(t0=500, t1=3071)), ("threshold", False, 8, "SAGITAL", dict(t0=1500, t1=3071)),
             ("threshold", False, 4, "CORONAL", dict(t0=-2000, t1=-1500)),  # click rejected
             ("dynamic", False, 8, "CORONAL", dict(dev_min=400, dev_max=300)), ("dynamic", True, 4, "SAGITAL", dict(dev_min=60, dev_max=40)),
             ("dynamic", True, 8, "AXIAL", dict(dev_min=60, dev_max=40)),
             ("confidence", False, 4, "AXIAL", {}), ("confidence", True, 8, "CORONAL", {}), ("confidence", False, 8, "SAGITAL", {})]
    meta, mats = [], []
    for method, use_ww_wl, con, ori, extra in cases:
        mat = mask_in.copy()
        s, cur = slice_ns(mat, img)
        s.window_width, s.window_level = 900, 400
        ax = ORIENTATIONS.index(ori)
        n = seed[2 - ax]
        xy = {"AXIAL": (seed[0], seed[1]), "CORONAL": (seed[0], seed[2]), "SAGITAL": (seed[1], seed[2])}[ori]
        s.buffer_slices[ori] = types.SimpleNamespace(mask=np.array(slice_of(mat[1:, 1:, 1:], ori, n)), image=slice_of(img, ori, n), index=n)
        cfg = types.SimpleNamespace(method=method, use_ww_wl=use_ww_wl, con_2d=con, fill_value=254, confid_mult=2.5, confid_iters=3,
                                    t0=0, t1=0, dev_min=0, dev_max=0)
        for k, v in extra.items():
            setattr(cfg, k, v)
        self_ = types.SimpleNamespace(config=cfg, picker=None, orientation=ori, GetMousePosition=lambda: (0, 0),
                                      viewer=types.SimpleNamespace(slice_=s, get_slice_pixel_coord_by_screen_pos=lambda mx, my, pk, xy=xy: xy))
        self_.do_rg_confidence = lambda *a, **k: rst.FloodFillSegmentInteractorStyle.do_rg_confidence(self_, *a, **k)
        rst.FloodFillSegmentInteractorStyle.do_2d_seg(self_)
        meta.append((("threshold", "dynamic", "confidence").index(method), int(use_ww_wl), con, ax, n, xy[0], xy[1], cfg.t0, cfg.t1,
                     cfg.dev_min, cfg.dev_max))
        mats.append(mat)
    d["seg2d_meta"], d["seg2d_out"] = np.array(meta), np.stack(mats)
    d["seg2d_wwwl"] = np.array([900, 400])

    # ---- CropMask ----------------------------------------------------------------------------------------------------------------------
    boxes = [(0, 5, 3, 19, 2, 4), (7, 7, 9, 9, 3, 3), (0, 23, 0, 19, 0, 8), (10, 23, 0, 6, 0, 8)]  # a face, one voxel, everything, a corner
    mats = []
    for k, box in enumerate(boxes):
        mat = np.memmap(os.path.join(tmp_root, "crop_%d.dat" % k), dtype=np.uint8, mode="w+", shape=mask_in.shape)  # (flush())
        mat[:] = mask_in
        s, cur = slice_ns(mat, img)
        cur.modified = lambda *a, **k: None
        s.do_threshold_to_all_slices = lambda s=s, cur=cur: rs.Slice.do_threshold_to_all_slices(s, cur, img)
        self_ = types.SimpleNamespace(viewer=types.SimpleNamespace(orientation="AXIAL", slice_=s),
                                      draw_retangle=types.SimpleNamespace(box=types.SimpleNamespace(GetLimits=lambda box=box: box)))
        rst.CropMaskInteractorStyle.CropMask(self_)
        mats.append(np.array(mat))
    d["crop_boxes"], d["crop_out"] = np.array(boxes), np.stack(mats)

    np.savez_compressed(path, **d)
    print(len(d), "arrays from the reference's own methods,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ref_editor.npz"))
