"""Golden vectors from the REFERENCE ITSELF for the volume renderer's host side: invesalius.data.volume.Volume imported
from a reference checkout, its VTK classes replaced by recorders, driven through LoadVolume (the first load of a
preset) and __load_preset (a preset switch) for all 30 raycasting presets at three scalar ranges, plus SetWWWL and
CalculateWWWL.

    python3 tests/golden/make_golden_ref_volume.py REFERENCE_DIR [OUT.npz]

The module's GUI-side imports (wx, vtk, pubsub, ...) are satisfied by the stand-in module finder of
make_golden_ref_dowatershed.py.  What is recorded:
  - every AddRGBPoint / AddPoint / AddSegment of the colour and opacity functions (__update_colour_table),
  - the vtkVolumeProperty calls (SetShading, the ShadeOn of LoadVolume) and the mapper's blend mode on both paths,
  - the vtkImageShiftScale shift and each vtkImageConvolve kernel,
  - the preset dict after SetWWWL and (ww, wl, curve) after CalculateWWWL for several (ww, wl, curve).
The scalar ranges are (-1024, 3071), (0, 1200) and (100, 1900): the last one shows the shift quirk (the data shift by
+scale[0] while the tables translate by -scale[0]).  The presets (as JSON) and the colour lists travel in the .npz, so
the tests never read a reference checkout.
"""
import copy
import glob
import json
import os
import plistlib
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ref_dowatershed as M  # noqa: E402  (the stand-in module finder)

SCALES = ((-1024, 3071), (0, 1200), (100, 1900))
LOG = []


class _Dummy:
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: _Dummy()


class _Recorder:
    """Records every method call as (class, method, args) in LOG."""
    kind = "?"

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*a, **k):
            LOG.append((self.kind, name, [x if isinstance(x, (int, float, str, bool)) else
                                          ([float(v) for v in x] if isinstance(x, (list, tuple)) else None) for x in a]))
            return _Dummy()
        return call


def _recorder(kind, **methods):
    return type("Rec_" + kind, (_Recorder,), dict(kind=kind, **methods))


def main(ref_dir, out):
    sys.meta_path.insert(0, M._Finder())
    import pubsub.pub
    pubsub.pub.subscribe = lambda *a, **k: (None, True)
    os.environ["HOME"] = tempfile.mkdtemp()
    sys.path.insert(0, ref_dir)
    import invesalius.data.volume as V

    presets_dir = os.path.join(ref_dir, "presets", "raycasting")
    V.inv_paths.RAYCASTING_PRESETS_DIRECTORY = presets_dir
    V.Publisher = types.SimpleNamespace(sendMessage=lambda *a, **k: None, subscribe=lambda *a, **k: None)
    V.vtk_utils = types.SimpleNamespace(ShowProgress=lambda *a, **k: (lambda *a, **k: None))
    V.ses = types.SimpleNamespace(Session=lambda: types.SimpleNamespace(GetConfig=lambda *a, **k: 0))
    scale_box = {}

    class _Image(_Recorder):
        kind = "image"

        def GetScalarRange(self):
            return scale_box["scale"]

    def _get_output(self):
        return _Image()

    prop_holder = {}

    def _get_property(self):
        return prop_holder["p"]

    def _prop_init(self):
        prop_holder["p"] = self

    V.vtkColorTransferFunction = _recorder("ctf")
    V.vtkPiecewiseFunction = _recorder("pwf")
    V.vtkVolumeProperty = _recorder("prop", __init__=_prop_init)
    V.vtkFixedPointVolumeRayCastMapper = _recorder("mapper", IsA=lambda self, n: n == "vtkFixedPointVolumeRayCastMapper")
    V.vtkVolume = _recorder("volume", GetProperty=_get_property)
    V.vtkImageFlip = _recorder("flip", GetOutput=_get_output)
    V.vtkImageShiftScale = _recorder("cast", GetOutput=_get_output)
    V.vtkImageConvolve = _recorder("convolve", GetOutput=_get_output)

    presets = {}
    for f in sorted(glob.glob(os.path.join(presets_dir, "*.plist"))):
        with open(f, "rb") as fh:
            presets[os.path.basename(f)[:-6]] = plistlib.load(fh, fmt=plistlib.FMT_XML)
    assert len(presets) == 30, len(presets)
    data = {"presets_json": np.array(json.dumps(presets)), "scales": np.array(SCALES, np.float64)}
    cluts = sorted({p["CLUT"] for p in presets.values() if not p["advancedCLUT"] and p["CLUT"] != "No CLUT"})
    for c in cluts:
        with open(os.path.join(presets_dir, "color_list", c + ".plist"), "rb") as fh:
            p = plistlib.load(fh, fmt=plistlib.FMT_XML)
        data["clut_" + c] = np.array(list(zip(p["Red"], p["Green"], p["Blue"])), np.float64)

    def tables(log):
        ctf = [[c[2][0], c[2][1], c[2][2], c[2][3]] for c in log if c[0] == "ctf" and c[1] == "AddRGBPoint"]
        pwf = [[0.0, c[2][0], c[2][1], 0.0, 0.0] if c[1] == "AddPoint" else [1.0] + list(c[2][:4])
               for c in log if c[0] == "pwf" and c[1] in ("AddPoint", "AddSegment")]
        return np.array(ctf, np.float64).reshape(-1, 4), np.array(pwf, np.float64).reshape(-1, 5)

    meta = {}
    names = sorted(presets)
    for i, name in enumerate(names):
        for j, scale in enumerate(SCALES):
            scale_box["scale"] = tuple(float(s) for s in scale)
            vol = V.Volume()
            vol.config = copy.deepcopy(presets[name])
            vol.loaded_image = True
            vol.image = _Image()
            LOG.clear()
            vol.LoadVolume()
            first = list(LOG)
            ctf, pwf = tables(first)
            data["%d_%d_ctf" % (i, j)] = ctf
            data["%d_%d_pwf" % (i, j)] = pwf
            LOG.clear()
            vol._Volume__load_preset()
            switch = list(LOG)
            ctf2, pwf2 = tables(switch)
            assert np.array_equal(ctf, ctf2) and np.array_equal(pwf, pwf2)
            meta["%d_%d" % (i, j)] = {
                "preset": name, "scale": list(scale),
                "prop_first": [c[1:] for c in first if c[0] == "prop" and c[1] != "SetColor" and c[1] != "SetScalarOpacity"],
                "prop_switch": [c[1:] for c in switch if c[0] == "prop"],
                "mapper_first": [c[1:] for c in first if c[0] == "mapper" and c[1].startswith("SetBlendMode")],
                "mapper_switch": [c[1:] for c in switch if c[0] == "mapper" and c[1].startswith("SetBlendMode")],
                "shift": [c[2] for c in first if c[0] == "cast" and c[1] == "SetShift"],
                "kernels": [c[2][0] for c in first if c[0] == "convolve" and c[1] == "SetKernel5x5"],
                "sample": [c[1:] for c in first if c[0] == "mapper" and c[1] in ("SetSampleDistance", "SetImageSampleDistance")]
                + [c[1:] for c in first if c[0] == "prop" and c[1] == "SetScalarOpacityUnitDistance"],
            }
    # SetWWWL / CalculateWWWL on 16-bit and 8-bit presets, curve indices in and past range
    wwwl = []
    for name in ("Bone + Skin", "Gold Bone", "MIP", "Airways", "Standard", "Vascular", "Black & White"):
        for ww, wl, curve in ((400.0, 40.0, 0), (1000.0, 300.0, 1), (250.5, -600.25, 0), (800.0, 500.0, 5)):
            vol = V.Volume()
            vol.config = copy.deepcopy(presets[name])
            vol.scale = SCALES[0]
            vol.curve = curve
            vol.SetWWWL(ww, wl)
            rec = {"preset": name, "ww": ww, "wl": wl, "curve": curve, "after": vol.config, "curve_after": vol.curve}
            if presets[name]["advancedCLUT"]:
                vol2 = V.Volume()
                vol2.config = copy.deepcopy(presets[name])
                vol2.curve = curve
                try:
                    vol2.CalculateWWWL()
                    rec["calc"] = [vol2.ww, vol2.wl, vol2.curve]
                except IndexError:  # the fallback steps back by one curve only
                    rec["calc"] = "IndexError"
            wwwl.append(rec)
    data["meta_json"] = np.array(json.dumps(meta))
    data["wwwl_json"] = np.array(json.dumps(wwwl))
    data["names_json"] = np.array(json.dumps(names))
    np.savez_compressed(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "ref_volume.npz"))
