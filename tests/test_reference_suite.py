"""The reference's OWN test files for this path, as far as the repository can carry them: tools/run_reference_tests.py --record
ran test_segmentation_tools.py, test_bone_thresholding.py and test_mask.py of the reference unmodified (23 passed), with
`invesalius_rs._native` (the Rust extension) bound to oracle/'s C restatement and `skimage.segmentation.watershed` to the real
scikit-image, and wrote down every call they made across that boundary: the arguments before the call, the arrays after it
and the value returned (tests/golden/ref_suite_calls.npz: data only, the outputs the reference's own assertions accepted).
Here every recorded call goes through the restatement again and must leave the same bits; tests/test_gpu_reference_calls.py
does the same through the product on the GPU."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_suite_calls.npz")


def _calls():
    z = np.load(GOLD)
    man = json.loads(str(z["manifest"]))

    def get(d):
        return None if d is None else (np.array(z[d["a"]]) if "a" in d else d["v"])
    return [(c["name"], [get(a) for a in c["args"]], [get(a) for a in c["after"]], get(c["ret"])) for c in man]


def test_recorded_reference_suite_calls_through_the_restated_native_code(oracle):
    from scipy import ndimage

    target = {"floodfill": oracle.floodfill, "floodfill_threshold": oracle.floodfill_threshold,
              "floodfill_threshold_inplace": oracle.floodfill_threshold_inplace,
              "floodfill_auto_threshold": oracle.floodfill_auto_threshold,
              "fill_holes_automatically": oracle.fill_holes_automatically,
              # scikit-image's heap flood, restated move for move (heap-ordered marker ties)
              "watershed": lambda image, markers, strct: oracle.watershed_sk(image, markers, strct, 0),
              "watershed_ift": ndimage.watershed_ift}
    calls = _calls()
    assert len(calls) >= 5
    seen = {}
    for name, args, after, ret in calls:
        live = [np.array(a, copy=True) if isinstance(a, np.ndarray) else
                ([tuple(s) for s in a] if name.startswith("floodfill") and isinstance(a, list) and a and isinstance(a[0], list) else a)
                for a in args]
        got = target[name](*live)
        for k, want in enumerate(after):
            if want is not None:
                assert live[k].dtype == want.dtype and np.array_equal(live[k], want), (name, k, int((live[k] != want).sum()))
        if isinstance(ret, np.ndarray):
            assert np.array_equal(np.asarray(got), ret), (name, "return", int((np.asarray(got) != ret).sum()))
        elif ret is not None:
            assert got == ret, (name, got, ret)
        seen[name] = seen.get(name, 0) + 1
    assert {"floodfill_threshold", "fill_holes_automatically", "watershed"} <= set(seen), seen
