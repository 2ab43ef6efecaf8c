"""Golden numbers from the REFERENCE ITSELF for the surface view: the three constants its own Python hands the
vtkActor of Surface._show_surface (invesalius/data/surface.py:1061-1116).  VTK's rendering is not recorded (it is not
installed; rules R1 - R5 are the project's statement of it).  The reference's modules are imported from its checkout
(INVESALIUS_REFERENCE) under the stand-in finder.

    INVESALIUS_REFERENCE=<the reference's checkout> python3 tests/golden/make_golden_ref_surfaceview.py

Recorded: const.SURFACE_TRANSPARENCY, the session's default "surface_interpolation" (session.CONFIG_INIT) and the
const.SURFACE_COLOUR list.  Numbers only.
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ref_dowatershed as M  # noqa: E402


def main(path):
    tmp_root = tempfile.mkdtemp(prefix="ref_surfaceview_")
    tempfile.tempdir = tmp_root
    os.environ["HOME"] = tmp_root
    sys.meta_path.insert(0, M._Finder())
    import pubsub.pub
    pubsub.pub.subscribe = lambda *a, **k: (None, True)
    pubsub.pub.sendMessage = lambda *a, **k: None
    reference = os.environ.get("INVESALIUS_REFERENCE")
    if not reference or not os.path.isdir(os.path.join(reference, "invesalius")):
        raise SystemExit("set INVESALIUS_REFERENCE to the reference's checkout (the directory that holds invesalius/)")
    sys.path.insert(0, reference)
    from invesalius import constants as const
    from invesalius import session
    d = {"SURFACE_TRANSPARENCY": float(const.SURFACE_TRANSPARENCY),
         "SURFACE_INTERPOLATION": int(session.CONFIG_INIT["surface_interpolation"]),
         "SURFACE_COLOUR": [[float(x) for x in c] for c in const.SURFACE_COLOUR]}
    with open(path, "w") as f:
        json.dump(d, f, indent=1)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(os.path.join(HERE, "ref_surfaceview.json"))
