"""Golden vectors from the REFERENCE ITSELF for the mask 3-D preview's host side: invesalius.data.volume_mask.VolumeMask
imported from a reference checkout, its VTK classes replaced by recorders, driven through create_volume and set_colour
for three colours with the session's ``rendering`` answering 0 (vtkFixedPointVolumeRayCastMapper) and 1
(vtkGPUVolumeRayCastMapper with the iso-surface blend mode).

    python3 tests/golden/make_golden_ref_maskpreview.py REFERENCE_DIR [OUT.npz]

The module's GUI-side imports are satisfied by the stand-in module finder of make_golden_ref_dowatershed.py;
``vtkVersion().GetVTKVersion()`` answers "9.3.0", the pinned version.  What is recorded, in call order, as
(class, method, arguments): every call on the mapper, the flip, the colour and opacity functions, the volume property,
its iso-surface values and the volume actor.  The .npz holds one JSON string, so the tests never read a checkout.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ref_dowatershed as M  # noqa: E402  (the stand-in module finder)

COLOURS = ((0.0, 1.0, 0.0), (0.33, 0.25, 0.9), (1.0, 0.5, 0.125))
LOG = []


def _plain(x):
    if isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, (list, tuple)):
        return [float(v) for v in x]
    return type(x).__name__


class _Recorder:
    """Records every method call as [class, method, args] in LOG; the answers of `returns` are recorders themselves."""
    kind = "?"
    returns = {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*a, **k):
            LOG.append([self.kind, name, [_plain(x) for x in a]])
            return self.returns[name]() if name in self.returns else None
        return call


def _recorder(kind, returns=None, **methods):
    return type("Rec_" + kind, (_Recorder,), dict(kind=kind, returns=returns or {}, **methods))


def main(ref_dir, out):
    sys.meta_path.insert(0, M._Finder())
    import pubsub.pub
    pubsub.pub.subscribe = lambda *a, **k: (None, True)
    os.environ["HOME"] = tempfile.mkdtemp()
    sys.path.insert(0, ref_dir)
    import invesalius.data.volume_mask as VM

    rendering = {"value": 0}
    VM.ses = types.SimpleNamespace(Session=lambda: types.SimpleNamespace(GetConfig=lambda key, *a: rendering[
        "value"] if key == "rendering" else None))
    VM.vtkVersion = lambda: types.SimpleNamespace(GetVTKVersion=lambda: "9.3.0")

    def is_a(name):
        def f(self, n):
            LOG.append([self.kind, "IsA", [n]])
            return n == name
        return f

    iso_values = _recorder("isovalues")
    VM.vtkFixedPointVolumeRayCastMapper = _recorder("mapper_fixedpoint", IsA=is_a("vtkFixedPointVolumeRayCastMapper"))
    VM.vtkGPUVolumeRayCastMapper = _recorder("mapper_gpu", IsA=is_a("vtkGPUVolumeRayCastMapper"))
    VM.vtkImageFlip = _recorder("flip")
    VM.vtkColorTransferFunction = _recorder("ctf")
    VM.vtkPiecewiseFunction = _recorder("pwf")
    VM.vtkVolumeProperty = _recorder("prop", returns={"GetIsoSurfaceValues": iso_values})
    VM.vtkVolume = _recorder("volume")

    runs = []
    for r in (0, 1):
        rendering["value"] = r
        for i, colour in enumerate(COLOURS):
            mask = types.SimpleNamespace(colour=colour, imagedata="imagedata")
            vm = VM.VolumeMask(mask)
            LOG.clear()
            vm.create_volume()
            rec = {"rendering": r, "colour": list(colour), "create_volume": [list(c) for c in LOG], "set_colour": []}
            LOG.clear()
            vm.create_volume()  # a second call builds nothing
            assert not LOG
            for j, other in enumerate(COLOURS):
                if j == i:
                    continue
                LOG.clear()
                vm.set_colour(other)
                rec["set_colour"].append({"colour": list(other), "calls": [list(c) for c in LOG]})
            runs.append(rec)
    np.savez_compressed(out, runs_json=np.array(json.dumps(runs)))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "ref_maskpreview.npz"))
