"""ctypes binding of libivx.so (the C ABI declared in include/ivx.h).

This is the stub a reference maintainer would add in place of ``from invesalius_rs import _native``
(invesalius_rs/__init__.py:8).  There is no CPU fallback: if the shared library is missing the import of any
compute entry point raises, and on a machine without a HIP device every call returns IVX_EHIP -> RuntimeError.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IVX_LIB_PATH") or os.path.join(_HERE, "libivx.so")  # IVX_LIB_PATH: A/B builds of the same ABI

IVX_OK, IVX_EINVAL, IVX_ERANGE, IVX_ENOMEM, IVX_EDOM, IVX_EHIP, IVX_ESTALE = 0, -1, -2, -3, -4, -5, -6
IVX_EINTERNAL = -7
U8, I16, F64, U16, F32, I32, I64, I8 = 0, 1, 2, 3, 4, 5, 6, 7
DT = {np.dtype(np.uint8): U8, np.dtype(np.int16): I16, np.dtype(np.float64): F64, np.dtype(np.uint16): U16, np.dtype(np.float32): F32, np.dtype(np.int32): I32,
      np.dtype(np.int64): I64}
MIP_MAX, MIP_MIN, MIP_MEAN, MIP_SUM = 0, 1, 2, 3

c_i64 = ctypes.c_int64
c_vp = ctypes.c_void_p


class McParams(ctypes.Structure):
    """struct ivx_mc_params (include/ivx.h)."""
    _fields_ = [
        ("dtype", ctypes.c_int32), ("pad_xy", ctypes.c_int32), ("pad_bottom", ctypes.c_int32),
        ("pad_top", ctypes.c_int32), ("vtk_pz", ctypes.c_int32), ("niso", ctypes.c_int32),
        ("nz", c_i64), ("ny", c_i64), ("nx", c_i64), ("roi_start", c_i64),
        ("pad_value", ctypes.c_double), ("spacing", ctypes.c_double * 3), ("iso", ctypes.c_double * 2),
    ]


class FloodPlan(ctypes.Structure):
    """struct ivx_flood_plan (include/ivx.h)."""
    _fields_ = [("dz", c_i64), ("dy", c_i64), ("dx", c_i64), ("wx", c_i64), ("strct_bits", ctypes.c_uint32)]


FLOOD_WRITE_NONE, FLOOD_WRITE_MASK_FROM_PLANES, FLOOD_WRITE_APPLY_LEVELS, FLOOD_WRITE_APPLY_U8 = 0, 1, 2, 3


class FloodWrite(ctypes.Structure):
    """struct ivx_flood_write (include/ivx.h): the write ivx_dev_flood_grow_select queues behind the flood"""
    _fields_ = [("kind", ctypes.c_int32), ("v_in", ctypes.c_int32), ("v_sel", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("inside_bits", c_vp), ("mask", c_vp)]


class VolrenParams(ctypes.Structure):
    """struct ivx_volren_params (include/ivx.h)."""
    _fields_ = [
        ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("mip", ctypes.c_int32), ("shade", ctypes.c_int32),
        ("skip", ctypes.c_int32), ("n_table", ctypes.c_int32), ("out_u8", ctypes.c_int32), ("clip", ctypes.c_int32),
        ("origin", ctypes.c_double * 3), ("du", ctypes.c_double * 3), ("dv", ctypes.c_double * 3),
        ("dir", ctypes.c_double * 3), ("spacing", ctypes.c_double * 3), ("dt", ctypes.c_double),
        ("ambient", ctypes.c_double), ("diffuse", ctypes.c_double), ("specular", ctypes.c_double),
        ("specular_power", ctypes.c_double), ("background", ctypes.c_double * 3), ("clip_normal", ctypes.c_double * 3),
        ("clip_origin", ctypes.c_double * 3),
    ]


ROI_ELLIPSE, ROI_POLYGON, ROI_MAX_POINTS, ROI_RECORD_BYTES = 0, 1, 2048, 40
# the words of the weld's counts (IVX_WELD_* of include/ivx.h)
WELD_COUNT_WORDS, WELD_VERTS, WELD_KEPT, WELD_DROPPED, WELD_OVERRUN, WELD_NONFINITE, WELD_MAX_PROBE, WELD_LOG2_SLOTS, WELD_HIST = 32, 0, 1, 2, 3, 4, 5, 6, 8
WELD_MAX_CORNERS = 2 ** 31 - 1


class Roi(ctypes.Structure):
    """struct ivx_roi (include/ivx.h): one region of interest of the density measures"""
    _fields_ = [
        ("image", c_vp), ("row_stride", c_i64), ("elem_stride", c_i64), ("h", c_i64), ("w", c_i64),
        ("kind", ctypes.c_int32), ("n_points", ctypes.c_int32), ("first_point", c_i64),
        ("sx", ctypes.c_double), ("sy", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double),
        ("a2", ctypes.c_double), ("b2", ctypes.c_double),
        ("x0", c_i64), ("y0", c_i64), ("x1", c_i64), ("y1", c_i64), ("first_block", c_i64), ("n_blocks", c_i64),
    ]


class StaleError(RuntimeError):
    """IVX_ESTALE: a registered host array (resident.bind) was written without a touch; raised only with the stale check on."""


def _declare(lib):
    """signatures of the resident-array calls (include/ivx.h): handles are 64-bit, sizes size_t"""
    u64, sz, u64p = ctypes.c_uint64, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)
    i64p = ctypes.POINTER(c_i64)
    for name, args in (("ivx_host_register", [c_vp, sz, u64p]), ("ivx_host_touch", [u64]), ("ivx_host_touch_range", [u64, sz, sz]),
                       ("ivx_host_release", [u64]), ("ivx_host_stats", [u64, u64p]), ("ivx_host_count", [u64p]),
                       ("ivx_host_set_check", [ctypes.c_int]), ("ivx_transfer_stats", [u64p]),
                       ("ivx_upload_strided", [c_vp, c_vp, i64p, i64p, sz]), ("ivx_download_strided", [c_vp, i64p, i64p, c_vp, sz]),
                       # the per-word (min, max) records of an int16 image and the kernels that read them
                       ("ivx_image_ranges_bytes", [c_i64, c_i64, c_i64, ctypes.POINTER(sz)]),
                       ("ivx_dev_image_ranges_i16", [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp]),
                       ("ivx_dev_threshold_i16_bits_ranges", [c_vp, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp,
                                                              ctypes.c_int, c_vp]),
                       # the plane-only thresholds and the pass that writes the mask's bytes from its planes
                       ("ivx_dev_threshold_i16_plane", [c_vp, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
                       ("ivx_dev_threshold_i16_plane_ranges", [c_vp, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int, c_vp, c_vp,
                                                               ctypes.c_int, c_vp]),
                       ("ivx_dev_mask_from_planes", [ctypes.POINTER(FloodPlan), c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, c_vp]),
                       ("ivx_dev_flood_candidates_ranges", [ctypes.POINTER(FloodPlan), c_vp, ctypes.c_double, ctypes.c_double, c_vp,
                                                            ctypes.c_int, ctypes.c_double, c_vp, c_vp, c_vp]),
                       # flood + the write of its result in one call: ..., rounds, write, look-ahead, stream
                       ("ivx_dev_flood_grow_select", [ctypes.POINTER(FloodPlan), ctypes.c_int, c_vp, ctypes.c_double, ctypes.c_double,
                                                      c_vp, c_i64, c_vp, c_vp, c_vp, ctypes.POINTER(ctypes.c_int),
                                                      ctypes.POINTER(FloodWrite), ctypes.c_int, c_vp]),
                       ("ivx_dev_flood_grow_select_count", [ctypes.POINTER(FloodPlan), ctypes.c_int, c_vp, ctypes.c_double, ctypes.c_double,
                                                            c_vp, c_i64, c_vp, c_vp, c_vp, ctypes.POINTER(ctypes.c_int),
                                                            ctypes.POINTER(FloodWrite), ctypes.c_int, ctypes.POINTER(McParams), c_vp,
                                                            ctypes.POINTER(ctypes.c_int), c_vp]),
                       ("ivx_flood_look_ahead", [c_i64, ctypes.POINTER(ctypes.c_int32)]),
                       # the image geometry tools (flip, swap axes, gantry tilt) and the calls that keep a mask's zeros off the link
                       ("ivx_dev_image_flip", [c_vp, c_i64, c_i64, c_i64, sz, ctypes.c_int, c_vp]),
                       ("ivx_image_flip", [c_vp, i64p, i64p, sz, ctypes.c_int]),
                       ("ivx_dev_image_swap_axes", [c_vp, c_i64, c_i64, c_i64, sz, ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
                       ("ivx_image_swap_axes", [c_vp, i64p, i64p, sz, ctypes.c_int, ctypes.c_int, c_vp, i64p]),
                       ("ivx_image_tilt_scratch_bytes", [c_i64, c_i64, c_i64, ctypes.POINTER(sz)]),
                       ("ivx_dev_image_fix_gantry_tilt", [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, sz, c_vp, c_vp]),
                       ("ivx_image_fix_gantry_tilt", [c_vp, i64p, i64p, c_vp, c_vp]),
                       ("ivx_host_zero", [c_vp, sz]), ("ivx_host_register_zero", [c_vp, sz, u64p]),
                       # the slice display: three 2-D views (pointer, row stride, element stride), h, w, parameters, tables, out
                       ("ivx_slice_show_tables_bytes", [ctypes.c_int, ctypes.POINTER(sz)]),
                       ("ivx_dev_slice_show", [c_vp, c_i64, c_i64] * 3 + [c_i64, c_i64, c_vp, c_vp, c_vp, c_vp]),
                       ("ivx_slice_show", [c_vp, c_i64, c_i64] * 3 + [c_i64, c_i64, c_vp, c_vp, c_vp]),
                       # the mask edit history's volume snapshots (blocks64): header size, scan / pack / restore, host forms
                       ("ivx_mask_snapshot_header_bytes", [c_i64, ctypes.POINTER(sz)]),
                       ("ivx_dev_mask_snapshot_scan", [c_vp, c_i64, c_vp, i64p, c_vp]),
                       ("ivx_dev_mask_snapshot_pack", [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
                       ("ivx_dev_mask_snapshot_restore", [c_vp, c_i64, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp]),
                       ("ivx_mask_snapshot", [c_vp, sz, ctypes.POINTER(c_vp), ctypes.POINTER(c_vp), i64p]),
                       ("ivx_mask_snapshot_restore", [c_vp, sz, c_vp, c_vp, c_i64, sz, i64p]),
                       # the surface view: mesh, camera, stages, keys; layers, camera, mode, background, out_u8, picture, ids, depth
                       ("ivx_dev_surface_raster", [c_vp, c_i64, c_vp, c_i64, c_vp, ctypes.c_int, c_vp, c_vp]),
                       ("ivx_dev_surface_resolve", [c_vp, ctypes.c_int, c_vp, ctypes.c_int, c_vp, ctypes.c_int, c_vp, c_vp, c_vp, c_vp]),
                       ("ivx_surface_render", [c_vp, ctypes.c_int, c_vp, ctypes.c_int, c_vp, ctypes.c_int, c_vp, c_vp, c_vp]),
                       # the 3-D scene: field kind, field, cells, shape, strides, apron, apron value, table, prefix, layers, count,
                       # camera, interpolation, planes, count, params, out, stats, stream; host form
                       ("ivx_dev_scene_render", [ctypes.c_int, c_vp, c_vp, i64p, i64p, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp, ctypes.c_int,
                                                 c_vp, ctypes.c_int, c_vp, ctypes.c_int, c_vp, c_vp, c_vp, c_vp]),
                       ("ivx_scene_render", [ctypes.c_int, c_vp, i64p, i64p, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp, ctypes.c_int, c_vp,
                                             ctypes.c_int, c_vp, ctypes.c_int, c_vp, c_vp]),
                       # the density measures: descriptors, count, points (host; device), count, records
                       ("ivx_dev_roi_density", [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp]),
                       ("ivx_roi_density", [c_vp, c_i64, c_vp, c_i64, c_vp]),
                       # the 3-D mask editor: screen filter, cut, brush stroke, equal, apply; host forms
                       ("ivx_dev_m3e_filter", [c_i64, c_i64, c_vp, c_vp, c_i64, ctypes.c_int, c_vp, c_vp]),
                       ("ivx_dev_m3e_cut", [c_vp, i64p, i64p, c_vp, ctypes.c_double, c_vp, c_i64, c_i64, c_vp, c_vp, ctypes.c_int, c_vp, c_vp]),
                       ("ivx_dev_m3e_brush_stroke", [c_vp, c_vp, i64p, i64p, c_vp, c_vp, c_vp, c_i64, ctypes.c_double, ctypes.c_int, c_vp,
                                                     c_vp]),
                       ("ivx_dev_m3e_equal", [c_vp, c_vp, c_i64, ctypes.POINTER(ctypes.c_int), c_vp]),
                       ("ivx_dev_m3e_apply", [c_vp, c_vp, i64p, i64p, c_vp, c_vp]),
                       ("ivx_m3e_filter", [c_i64, c_i64, c_vp, c_vp, c_i64, ctypes.c_int, c_vp]),
                       ("ivx_m3e_cut", [c_vp, i64p, i64p, c_vp, ctypes.c_double, c_vp, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp,
                                        ctypes.c_int, i64p]),
                       ("ivx_m3e_brush_stroke", [c_vp, c_vp, i64p, i64p, c_vp, c_vp, c_i64, ctypes.c_double, ctypes.c_int, i64p]),
                       ("ivx_m3e_apply", [c_vp, c_vp, i64p, i64p, i64p]), ("ivx_m3e_flag_planes", [c_vp, i64p, i64p]),
                       # surface import: table size, scratch size, weld, STL unpack, point transform; host forms
                       ("ivx_mesh_weld_slots", [c_i64, u64p]), ("ivx_mesh_weld_bytes", [c_i64, ctypes.POINTER(sz)]),
                       ("ivx_dev_mesh_weld", [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
                       ("ivx_dev_stl_unpack", [c_vp, c_i64, c_vp, c_vp, c_vp]),
                       ("ivx_dev_mesh_transform_points", [c_vp, c_i64, c_vp, c_vp, c_vp]),
                       ("ivx_mesh_weld", [c_vp, c_i64, c_vp, c_vp, c_vp]), ("ivx_mesh_stl_weld", [c_vp, sz, c_vp, c_vp, c_vp]),
                       ("ivx_mesh_transform_points", [c_vp, c_i64, c_vp, c_vp])):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, ctypes.c_int


_lib = None


def lib() -> ctypes.CDLL:
    """Load libivx.so (built in-tree by invesalius3_amd/build.py).  Fails loudly when absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libivx.so not found at %s: build it with `python -m invesalius3_amd.build` "
                "(there is no CPU fallback in this package)" % LIB_PATH)
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.ivx_last_error.restype = ctypes.c_char_p
        _declare(_lib)
    return _lib


def last_error() -> str:
    return (lib().ivx_last_error() or b"").decode("utf-8", "replace")


def check(rc: int, what: str = "ivx") -> int:
    """Map the C status to the exception the reference raises for the same condition."""
    if rc >= 0:
        return rc
    msg = "%s: %s" % (what, last_error())
    if rc == IVX_EINVAL:
        raise TypeError(msg)
    if rc == IVX_ERANGE:
        raise IndexError(msg)
    if rc == IVX_ENOMEM:
        raise MemoryError(msg)
    if rc == IVX_EDOM:
        raise ValueError(msg)
    if rc == IVX_ESTALE:
        raise StaleError(msg)
    raise RuntimeError(msg)


def i64(seq):
    return (c_i64 * len(seq))(*[int(v) for v in seq])


def ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data)


def dtype_code(a: np.ndarray, allowed=(U8, I16, F64, U16)) -> int:
    code = DT.get(a.dtype)
    if code is None or code not in allowed:
        raise TypeError("unsupported array dtype %s" % a.dtype)
    return code


class _Pinned:
    """owner of one hipHostMalloc block (freed when the last numpy view of it goes away)"""

    def __init__(self, nbytes: int):
        self.ptr = ctypes.c_void_p()
        check(lib().ivx_host_alloc(ctypes.byref(self.ptr), ctypes.c_size_t(int(nbytes))), "ivx_host_alloc")

    def __del__(self):
        try:
            if self.ptr and self.ptr.value:
                lib().ivx_host_free(self.ptr)
        except Exception:
            pass


def pinned_empty(shape, dtype) -> np.ndarray:
    """np.empty in page-locked host memory: uploads from it and downloads into it run at the PCIe link's rate (a pageable
    array goes through the runtime's bounce buffers).  For callers that can keep their volume / results there."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    own = _Pinned(max(n, 16))
    buf = (ctypes.c_uint8 * max(n, 16)).from_address(own.ptr.value)
    buf._ivx_owner = own  # the ctypes array keeps the block alive, numpy keeps the ctypes array alive
    return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)


def device_count() -> int:
    n = ctypes.c_int(0)
    lib().ivx_device_count(ctypes.byref(n))
    return n.value


def require_device():
    if device_count() < 1:
        raise RuntimeError("invesalius3_amd: no HIP device visible and there is no CPU fallback")


def device_name() -> str:
    buf = ctypes.create_string_buffer(256)
    check(lib().ivx_device_name(buf, ctypes.c_size_t(256)))
    return buf.value.decode()


def set_device(i: int):
    check(lib().ivx_set_device(int(i)))


def synchronize():
    check(lib().ivx_device_synchronize())


def flood_visits(plan: FloodPlan, scratch, stream=None):
    """(tile visits, length of the first round's list) of the last region-growing flood that ran on `scratch` (a device
    pointer): ivx_dev_flood_visits, queue-ordered on `stream`, one small read."""
    out = (ctypes.c_uint32 * 2)()
    check(lib().ivx_dev_flood_visits(ctypes.byref(plan), scratch, out, stream), "flood_visits")
    return int(out[0]), int(out[1])
