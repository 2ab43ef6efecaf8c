"""Golden vectors from the REFERENCE ITSELF for the image geometry tools: imagedata_utils.FixGantryTilt
(invesalius/data/imagedata_utils.py:143-154) over live scipy, and Slice.OnFlipVolume / Slice.OnSwapVolumeAxes
(invesalius/data/slice_.py:2103-2251).  The reference's modules are imported from its checkout (INVESALIUS_REFERENCE) under the
stand-in finder of make_golden_ref_dowatershed.py.  The two Slice methods are called unbound on a plain namespace that holds
the matrix, with ``Project()`` answering with a namespace of image versions and masks; the masks are stand-ins with the three
members the methods touch (``matrix``, ``_recreate_mask_matrix``, ``clear_history``), so what is recorded of them is the
shape the reference asks for and that every byte is zero.  OnSwapVolumeAxes writes its result to a temporary memmap, which is
read back here.

    INVESALIUS_REFERENCE=<the reference's checkout> python3 tests/golden/make_golden_ref_imagetools.py [out.npz]

The inputs come from tests/_imagegeo_cases.py and are stored next to the outputs.
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
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import make_golden_ref_dowatershed as M  # noqa: E402
import _imagegeo_cases as C  # noqa: E402

SWAPS = ((2, 1), (2, 0), (1, 0))
FLIP_SHAPE = (5, 6, 9)
SPACING = (0.5, 0.75, 2.0)


def reference_modules(reference):
    """(imagedata_utils, slice_) of the reference under the stand-ins"""
    tmp_root = tempfile.mkdtemp(prefix="ref_imagetools_")  # the reference's temporary files and its HOME: outside the tree
    tempfile.tempdir = tmp_root
    os.environ["HOME"] = tmp_root
    sys.meta_path.insert(0, M._Finder())
    import pubsub.pub
    pubsub.pub.subscribe = lambda *a, **k: (None, True)
    pubsub.pub.sendMessage = lambda *a, **k: None
    sys.path.insert(0, reference)
    from invesalius.data import imagedata_utils as riu
    from invesalius.data import slice_ as rs
    rs.ses = mock.MagicMock()
    rs.Publisher.sendMessage = lambda *a, **k: None
    return riu, rs


class _Flushable(np.ndarray):
    def flush(self):  # (the reference's mask matrices are memmaps)
        pass


class _Mask:
    def __init__(self, shape):
        self.matrix = np.full(shape, 7, np.uint8).view(_Flushable)
        self.cleared = 0

    def _recreate_mask_matrix(self, shape):
        self.matrix = np.zeros(shape, np.uint8).view(_Flushable)

    def clear_history(self):
        self.cleared += 1


def main(path):
    reference = os.environ.get("INVESALIUS_REFERENCE")
    if not reference or not os.path.isdir(os.path.join(reference, "invesalius")):
        raise SystemExit("set INVESALIUS_REFERENCE to the reference's checkout (the directory that holds invesalius/)")
    riu, rs = reference_modules(reference)
    d = {}

    # ---- FixGantryTilt ----------------------------------------------------------------------------------------------------------
    phantoms = {"disc": C.disc_phantom(), "slice0": C.slice0_min_phantom(), "wave": C.disc_phantom((5, 64, 64), seed=13)}
    d["tilts"] = np.array(C.TILTS)
    d["tilt_spacing"] = np.array(C.PHANTOM_SPACING)
    for name, vol in phantoms.items():
        d["tilt_in_" + name] = vol
        for t in C.TILTS:
            m = vol.copy()
            riu.FixGantryTilt(m, C.PHANTOM_SPACING, t)
            d["tilt_out_%s_%g" % (name, t)] = m

    # ---- OnFlipVolume / OnSwapVolumeAxes ----------------------------------------------------------------------------------------
    rng = np.random.default_rng(5)
    image = rng.integers(-1024, 3000, size=FLIP_SHAPE).astype(np.int16)
    version = rng.integers(-1024, 3000, size=FLIP_SHAPE).astype(np.int16)
    d["geo_in"], d["geo_version_in"], d["geo_spacing"] = image, version, np.array(SPACING)
    mask_shape = tuple(s + 1 for s in FLIP_SHAPE)
    buffers = {"AXIAL": types.SimpleNamespace(discard_buffer=lambda: None)}
    for axis in range(3):
        mask = _Mask(mask_shape)
        proj = types.SimpleNamespace(image_versions=[("original", None), ("Filtered 1", version.copy())], mask_dict={0: mask})
        self_ = types.SimpleNamespace(matrix=image.copy(), buffer_slices=buffers)
        proj.image_versions[0] = ("original", self_.matrix)
        with mock.patch.object(rs, "Project", lambda: proj):
            rs.Slice.OnFlipVolume(self_, axis)
        assert not mask.matrix.any() and mask.cleared == 1
        d["flip_out_%d" % axis], d["flip_version_out_%d" % axis] = self_.matrix, proj.image_versions[1][1]
    for a, b in SWAPS:
        mask = _Mask(mask_shape)
        fd, fname = tempfile.mkstemp()
        os.close(fd)
        m0 = image.copy()
        proj = types.SimpleNamespace(image_versions=[("Filtered 1", version.copy())], mask_dict={0: mask}, original_orientation=1)
        self_ = types.SimpleNamespace(matrix=m0, _matrix=m0, _matrix_filename=fname, spacing=SPACING, buffer_slices=buffers)
        with mock.patch.object(rs, "Project", lambda: proj):
            rs.Slice.OnSwapVolumeAxes(self_, (a, b))
        assert not mask.matrix.any() and mask.cleared == 1
        key = "%d%d" % (a, b)
        d["swap_out_" + key] = np.array(self_._matrix)
        d["swap_version_out_" + key] = np.array(proj.image_versions[0][1])
        d["swap_spacing_" + key] = np.array(self_.spacing)
        d["swap_mask_shape_" + key] = np.array(mask.matrix.shape)
        assert tuple(proj.matrix_shape) == self_._matrix.shape and tuple(proj.spacing) == tuple(self_.spacing)
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path), "bytes;", len(d), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ref_imagetools.npz"))
