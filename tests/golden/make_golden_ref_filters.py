"""Golden vectors from the REFERENCE ITSELF for the Image Filters dialog: the six functions of invesalius/data/filters.py
(5-66) run through Slice.__apply_image_filter's own `_run_filter` dispatch (invesalius/data/slice_.py:2330-2430), 3-D and
2-D for each orientation, imported from the reference checkout and called here.

    python3 tests/golden/make_golden_ref_filters.py REFERENCE_DIR [OUT.npz]   # stand-in modules for the GUI imports

`__apply_image_filter` is called unbound with a plain namespace as `self`; its worker thread is run synchronously (a
stand-in `threading.Thread`) and `Project()` is a namespace whose image_versions list is already non-empty, so no
memmap of the original is written.  The result is what the dispatch stashes in `_pending_filter_result`.  Border
detection with normalize=False is not reachable through the dispatch; it is taken from filters.border_detection_filter.

Keys: `vol_<v>` the inputs; `case_names` "<v>|<filter_type>|<value>|<dimension>|<orientation>" with `out_<i>` the
dispatch's result for case i; `nonorm_<v>_<value>` border_detection_filter(vol, value, normalize=False); `img2d` a 2-D
image and `img2d_<filter_type>_<value>` the six functions applied to it directly.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ref_dowatershed as M  # noqa: E402  (the stand-in module finder)

VALUES = {0: (0.1, 1.0, 2.5, 10.0), 1: (1.0, 1.6, 3.0), 2: (0.0, 0.5, 3.0, 15.0), 3: (0.3, 4.7), 4: (1.0, 10.0), 5: (1.0, 2.5)}
DIMS = (("3D", "Axial"), ("2D", "Axial"), ("2D", "Coronal"), ("2D", "Sagittal"))


def volumes():
    rng = np.random.default_rng(20261016)
    z, y, x = np.meshgrid(np.arange(7), np.arange(9), np.arange(11), indexing="ij")
    a = 900.0 * np.exp(-((z - 3) ** 2 + (y - 4) ** 2 + (x - 6) ** 2) / 8.0) + rng.normal(0, 60, (7, 9, 11)) - 200
    b = rng.integers(-1024, 3072, size=(3, 1, 12))  # 1-voxel axis, axes shorter than the radius
    c = np.full((4, 5, 6), 117)                     # constant: Mmax == Mmin
    return {"a": np.clip(a, -1024, 3071).astype(np.int16), "b": b.astype(np.int16), "c": c.astype(np.int16)}


def main(ref, path):
    sys.meta_path.insert(0, M._Finder())
    import pubsub.pub
    pubsub.pub.subscribe = lambda *a, **k: (None, True)
    pubsub.pub.sendMessage = lambda *a, **k: None
    os.environ.setdefault("HOME", tempfile.mkdtemp())
    sys.path.insert(0, ref)
    from invesalius.data import filters as rf
    from invesalius.data import slice_ as rs

    class _SyncThread:
        def __init__(self, target=None, daemon=None):
            self.target = target

        def start(self):
            self.target()

    rs.threading = types.SimpleNamespace(Thread=_SyncThread)
    rs.Project = lambda: types.SimpleNamespace(image_versions=[("original", None)], image_versions_meta={})
    apply = getattr(rs.Slice, "_Slice__apply_image_filter")
    d, names = {}, []
    vols = volumes()
    for vn, vol in vols.items():
        d["vol_" + vn] = vol
        for ft, values in VALUES.items():
            for v in values:
                for dim, ori in DIMS:
                    me = types.SimpleNamespace(matrix=vol, _matrix=vol, _is_filtering=False, _after_filter=lambda *a, **k: None)
                    apply(me, ft, v, dim, ori)
                    res = me._pending_filter_result
                    assert res is not None and res.dtype == np.int16 and res.shape == vol.shape
                    d["out_%d" % len(names)] = res
                    names.append("%s|%d|%r|%s|%s" % (vn, ft, v, dim, ori))
        for v in VALUES[5]:
            d["nonorm_%s_%r" % (vn, v)] = rf.border_detection_filter(vol, value=v, normalize=False)
    img2d = vols["a"][3]
    d["img2d"] = img2d
    fns = {0: rf.gaussian_blur_filter, 1: rf.median_blur_filter, 2: rf.mean_blur_filter, 3: rf.sharpening_filter,
           4: rf.despeckle_filter, 5: rf.border_detection_filter}
    for ft, values in VALUES.items():
        for v in values:
            d["img2d_%d_%r" % (ft, v)] = fns[ft](img2d, v)
    d["case_names"] = np.array(names)
    np.savez_compressed(path, **d)
    print("wrote %s: %d dispatch cases" % (path, len(names)))


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "ref_filters.npz"))
