"""Mask 3-D preview: the uint8 mask ray-cast as a shaded solid, in the two modes of the reference.

Restates invesalius/data/volume_mask.py:36-119 (``VolumeMask.create_volume`` / ``set_colour``) and the geometry of
``Mask.as_vtkimagedata`` (mask.py:294-313 with converters.to_vtk_mask, converters.py:104-136) with numpy only.  The render
contract the kernels of csrc/k_maskren.hip implement is in DESIGN.md section 7e; ``preview_setup`` holds what the
reference sets on its VTK objects, ``render_setup`` turns it and a camera into the numbers the kernels take.

VTK is not installed where this was written.  vtkVolumeProperty's default ambient (0.1) and diffuse (0.7), which the
reference leaves untouched, and the whole iso-surface contract of vtkGPUVolumeRayCastMapper (sample distance, first
crossing, one linear step) are restated from VTK's documentation, unverified.  The reference's jittering is not restated.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import volume as V

ISO_VALUE = 127            # GetIsoSurfaceValues().SetValue(0, 127), volume_mask.py:103
MODES = ("composite", "iso")  # session "rendering" 0 (the default) and 1
AMBIENT, DIFFUSE = 0.1, 0.7   # vtkVolumeProperty's defaults (unverified)
SPECULAR, SPECULAR_POWER = 0.75, 2.0  # volume_mask.py:96-97
N_TABLE = 257              # one entry per byte value and one more, so that a sample at 255 interpolates


def colour_nodes(colour) -> V.Nodes:
    """create_volume / set_colour (volume_mask.py:80-84, 113-119)"""
    r, g, b = [float(c) for c in colour]
    n = V.Nodes()
    n.add(0.0, 0, 0, 0)
    n.add(254.0, r, g, b)
    n.add(255.0, r, g, b)
    return n


def opacity_nodes() -> V.Nodes:
    """volume_mask.py:86-89"""
    n = V.Nodes()
    n.add(0.0, 0.0)
    n.add(127, 1.0)
    return n


def preview_setup(colour, mode: str = "composite") -> dict:
    """What create_volume sets for a mask of `colour` (r, g, b in 0..1): the transfer-function nodes, the volume
    property and the mapper of `mode` ("composite": vtkFixedPointVolumeRayCastMapper, session rendering 0; "iso":
    vtkGPUVolumeRayCastMapper with the iso-surface blend mode, rendering 1).  A value the reference does not set in a
    mode is None."""
    if mode not in MODES:
        raise ValueError("unknown mask preview mode %r (one of %s)" % (mode, ", ".join(MODES)))
    iso = mode == "iso"
    return {
        "mode": mode, "colour": tuple(float(c) for c in colour),
        "colour_nodes": colour_nodes(colour), "opacity_nodes": opacity_nodes(),
        "shade": True, "interpolation": "linear", "ambient": AMBIENT, "diffuse": DIFFUSE, "specular": SPECULAR,
        "specular_power": SPECULAR_POWER,
        "mapper": "vtkGPUVolumeRayCastMapper" if iso else "vtkFixedPointVolumeRayCastMapper",
        "blend": "iso_surface" if iso else "composite",
        "jitter": iso,  # UseJitteringOn: recorded, not restated
        "intermix_geometry": not iso,  # IntermixIntersectingGeometryOn: the geometry comes in through scene3d.Scene3D
        "iso_value": ISO_VALUE if iso else None,
        # pix_diag = 2.0: SetSampleDistance(pix_diag / 5.0), SetScalarOpacityUnitDistance(pix_diag); the image sample
        # distance is without effect, as for the image's volume
        "sample_distance": None if iso else V.SAMPLE_DISTANCE,
        "image_sample_distance": None if iso else 0.25,
        "opacity_unit_distance": None if iso else V.OPACITY_UNIT_DISTANCE,
    }


# -- geometry ---------------------------------------------------------------------------------------------------------
def voxel_world(index_zyx, spacing):
    """World position of matrix voxel (z, y, x): to_vtk_mask moves the origin by one spacing and the flip about the
    origin negates y, so the flag planes sit at -1 and ``matrix[1:, 1:, 1:]`` on the image's voxels."""
    z, y, x = [np.asarray(v, np.float64) for v in index_zyx]
    sx, sy, sz = [float(s) for s in spacing]
    return np.stack([(x - 1) * sx, -(y - 1) * sy, (z - 1) * sz], -1)


def preview_bounds(matrix_shape, spacing):
    """The box the rays are cut to, (xmin, xmax, ymin, ymax, zmin, zmax): the bounds of the voxel centres of the whole
    matrix, so the flag planes close the near faces and nothing closes the far ones (the reference's asymmetry)."""
    mz, my, mx = matrix_shape
    sx, sy, sz = [float(s) for s in spacing]
    return (-sx, (mx - 2) * sx, -(my - 2) * sy, sy, -sz, (mz - 2) * sz)


def default_sample_distance(spacing, mode: str) -> float:
    """composite: the reference's 2.0 / 5; iso: half the smallest spacing (unverified)"""
    return V.SAMPLE_DISTANCE if mode == "composite" else 0.5 * min(float(s) for s in spacing)


def render_setup(colour, mode, camera: dict, spacing, background=(0.0, 0.0, 0.0), sample_distance=None) -> dict:
    """`preview_setup` and a camera (volume.camera_for_view on the IMAGE's shape) as the numbers the kernels take, in the
    layout of volume.render_setup.  The rays' origin is moved by (sx, -sy, sz): index = world / spacing + 1 on the
    padded matrix, and a translation leaves the distances along the rays as they are."""
    ps = preview_setup(colour, mode)
    dt = float(default_sample_distance(spacing, mode) if sample_distance is None else sample_distance)
    if not dt > 0.0:
        raise ValueError("sample distance %r must be positive" % (sample_distance,))
    # the iso mode reads the colour at 127 only and takes the opacity there, 1, as it is
    rgba, alpha, prefix = V.bake_table(ps["colour_nodes"], ps["opacity_nodes"], N_TABLE - 2, dt,
                                       V.OPACITY_UNIT_DISTANCE if mode == "composite" else dt)
    origin, du, dv = V.pixel_rays(camera)
    sx, sy, sz = [float(s) for s in spacing]
    return {"preview": ps, "mode": mode, "iso": mode == "iso", "rgba": rgba, "alpha": alpha, "prefix": prefix,
            "mip": False, "shade": ps["shade"], "ambient": ps["ambient"], "diffuse": ps["diffuse"],
            "specular": ps["specular"], "specular_power": ps["specular_power"],
            "background": tuple(float(c) for c in background), "origin": origin + np.array([sx, -sy, sz]), "du": du,
            "dv": dv, "dir": camera["dir"], "viewport": camera["viewport"], "dt": dt, "clip": None}


def device_tables(setup: dict):
    """the baked table as the kernels read it: float32 (257, 4) and uint32 (258,)"""
    return np.ascontiguousarray(setup["rgba"], np.float32), np.ascontiguousarray(setup["prefix"], np.uint32)


def mask_preview(matrix: np.ndarray, spacing, colour, view="iso", size=(512, 512), mode: str = "composite",
                 background=(0.0, 0.0, 0.0), sample_distance=None, depth: bool = False, rgba8: bool = False):
    """Host form (ivx_mask_preview): the padded uint8 mask matrix (flag planes at index 0, any strides) over PCIe,
    rendered as `mode` from a standard `view` (or a camera dict from volume.camera_for_view on the image's shape);
    returns (H, W, 4) float32 RGBA, or uint8 with `rgba8`; with `depth` (iso mode) also the (H, W) float32 distance of
    the hit from the pixel's plane, +inf where nothing was hit."""
    from . import _lib as L

    if matrix.dtype != np.uint8 or matrix.ndim != 3 or min(matrix.shape) < 2:
        raise TypeError("matrix must be a 3-D uint8 array with its flag planes (every axis >= 2)")
    if depth and mode != "iso":
        raise ValueError("depth is an output of the iso mode")
    shape = tuple(int(s) - 1 for s in matrix.shape)
    cam = V.resolve_camera(view, shape, spacing, size)
    setup = render_setup(colour, mode, cam, spacing, background, sample_distance)
    rgba, prefix = device_tables(setup)
    p = V.volren_params(setup, spacing, rgba8)
    w, h = setup["viewport"]
    out = np.empty((h, w, 4), np.uint8 if rgba8 else np.float32)
    dep = np.empty((h, w), np.float32) if depth else None
    L.check(L.lib().ivx_mask_preview(L.ptr(matrix), L.i64(matrix.shape), L.i64(matrix.strides), int(setup["iso"]),
                                     L.ptr(rgba), L.ptr(prefix), ctypes.byref(p), L.ptr(out),
                                     None if dep is None else L.ptr(dep)), "mask_preview")
    return (out, dep) if depth else out
