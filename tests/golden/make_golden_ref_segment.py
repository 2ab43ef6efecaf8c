"""Golden vectors from the REFERENCE ITSELF for the deep-learning segmentation: segment_torch (segment.py:162-191, with
its gen_patches and the Unet3D of model.py) and SegmentProcess.apply_segment_threshold (segment.py:465-490), imported
from the reference checkout and run here on real torch (CPU, float32).

    python3 tests/golden/make_golden_ref_segment.py REFERENCE_DIR [OUT.npz]

The GUI-side imports are satisfied by the stand-in modules of make_golden_ref_dowatershed.py, except torch, which is the
real one.  The weights are tests/_unet_ref.make_weights() (seeded numpy, the reference's key names), written with
torch.save({"model_state_dict": ...}) to a temporary .pt that segment_torch loads itself.  apply_segment_threshold is
called unbound with a namespace `self` whose mask matrix is a memmap (the method flushes it).  apply_wwwl goes through
the reference's imagedata_utils.get_LUT_value first, as _run_segmentation does.

Keys: `param_names`, `param_shapes` (flattened, -1 separated), `weights_crc`; `cut_cases` "z,y,x|overlap|patch" with
`cuts_<i>` (n, 6) int32 (iz, ez, iy, ey, ix, ex); per segmentation case <c> in `seg_cases` ("name|patch|overlap|wwwl|ww|wl"):
`vol_<c>` the int16 image, `prob_<c>` the probability map, `mask_<c>` the mask after apply_segment_threshold(0.75).
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_ref_dowatershed as M  # noqa: E402  (the stand-in module finder)
import _unet_ref as R  # noqa: E402

CUT_SHAPES = ((48, 48, 48), (47, 49, 50), (10, 20, 30), (96, 100, 17), (1, 64, 200), (33, 33, 33), (16, 16, 16),
              (64, 32, 128), (120, 45, 61), (5, 5, 5), (50, 60, 70), (256, 31, 97))


class _Finder(M._Finder):
    ROOTS = tuple(r for r in M._Finder.ROOTS if r != "torch")


def seg_cases():
    rng = np.random.default_rng(20261017)
    wrap = rng.integers(-20000, 20000, (14, 18, 20)).astype(np.int16)
    wrap[0, 0, 0], wrap[-1, -1, -1] = -20000, 20000
    return [
        ("a", R.ct_volume((24, 40, 45), 31), 32, 50, False, 255, 127),  # z shorter than the patch
        ("wwwl", R.ct_volume((20, 18, 22), 32), 16, 50, True, 400, 40),
        ("wrap", wrap, 16, 25, False, 255, 127),  # range > 32767: both int16 wraps
        ("const", np.full((12, 14, 16), -77, np.int16), 16, 0, False, 255, 127),
    ]


def main(ref, path):
    sys.meta_path.insert(0, _Finder())
    import pubsub.pub
    pubsub.pub.subscribe = lambda *a, **k: (None, True)
    pubsub.pub.sendMessage = lambda *a, **k: None
    os.environ.setdefault("HOME", tempfile.mkdtemp())
    sys.path.insert(0, ref)
    import torch
    from invesalius.data import imagedata_utils as iu
    from invesalius.segmentation.deep_learning import segment as rseg
    from invesalius.segmentation.deep_learning.model import Unet3D

    torch.manual_seed(0)
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    d = {}
    # the reference's own key names and shapes
    ref_sd = Unet3D().state_dict()
    d["param_names"] = np.array(list(ref_sd.keys()))
    d["param_shapes"] = np.array([s for v in ref_sd.values() for s in list(v.shape) + [-1]], np.int32)
    sd = R.make_weights()
    assert list(sd) == list(ref_sd), "make_weights() does not follow Unet3D().state_dict()"
    d["weights_crc"] = np.array(R.weights_crc(sd), np.uint32)
    # gen_patches' cuts
    names = []
    for shp in CUT_SHAPES:
        for ov in (0, 10, 25, 50):
            for P in (16, 32, 48):
                img = np.zeros(shp, np.float32)
                cuts = [c for _, _, c in rseg.gen_patches(img, P, ov)]
                d["cuts_%d" % len(names)] = np.array([[a for ax in c for a in ax] for c in cuts], np.int32)
                names.append("%d,%d,%d|%d|%d" % (shp + (ov, P)))
    d["cut_cases"] = np.array(names)
    with tempfile.TemporaryDirectory() as tmp:
        wfile = os.path.join(tmp, "weights.pt")
        torch.save({"model_state_dict": {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}}, wfile)
        from pathlib import Path
        cases = []
        for name, vol, P, ov, wwwl, ww, wl in seg_cases():
            image = iu.get_LUT_value(vol, ww, wl) if wwwl else vol
            prob = np.zeros(vol.shape, np.float32)
            comm = np.zeros(1, np.float32)
            rseg.segment_torch(image, Path(wfile), ov, "cpu", prob, comm, P)
            assert comm[0] == np.inf
            mm = np.memmap(os.path.join(tmp, "m_%s.dat" % name), np.uint8, "w+", shape=tuple(s + 1 for s in vol.shape))
            me = types.SimpleNamespace(create_new_mask=True, _probability_array=prob,
                                       mask=types.SimpleNamespace(matrix=mm, was_edited=False, modified=lambda *a: None))
            rseg.SegmentProcess.apply_segment_threshold(me, 0.75)
            frac = float((prob >= np.float32(0.75)).mean())
            print("%s: p in [%.4f, %.4f], %.1f %% >= 0.75" % (name, prob.min(), prob.max(), 100 * frac))
            d["vol_" + name], d["prob_" + name], d["mask_" + name] = vol, prob, np.array(mm)
            cases.append("%s|%d|%d|%d|%d|%d" % (name, P, ov, int(wwwl), ww, wl))
        d["seg_cases"] = np.array(cases)
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "ref_segment.npz"))
