"""Threshold and slab-projection entry points of ``invesalius.data.slice_.Slice`` on the GPU.

The reference methods live on the ``Slice`` singleton and read GUI state; the compute part is restated here as
free functions with the state passed explicitly (mask matrix, image matrix, threshold range), same argument
meaning, same in-place effects on the caller-owned ``(dz+1, dy+1, dx+1)`` uint8 mask matrix
(invesalius/data/mask.py:422-431) including the per-slice flag cells ``matrix[n, 0, 0]``.
"""
from __future__ import annotations

import ctypes
import math
from fractions import Fraction

import numpy as np

from . import _lib as L
from . import resident

PROJECTION_NORMAL, PROJECTION_MaxIP, PROJECTION_MinIP, PROJECTION_MeanIP = 0, 1, 2, 3  # invesalius/constants.py:803-806


def bind_image(matrix: np.ndarray) -> "resident.Resident":
    """Keep the project's image in HBM: call it where the reference sets ``Slice.matrix`` (invesalius/data/slice_.py:175-188).
    Every entry point of this package that is then handed `matrix`, a slab or any other view of it uploads nothing; whoever
    writes the array with numpy calls ``touch`` on the returned `Resident` (resident.py, INTEGRATION.md "Resident arrays")."""
    return resident.bind(matrix)


def _int_bounds(threshold_range):
    """numpy compares int16 voxels with python numbers; for integer voxels `v >= lo` == `v >= ceil(lo)`."""
    lo, hi = threshold_range
    lo = int(math.ceil(lo))
    hi = int(math.floor(hi))
    lo = max(min(lo, 2 ** 31 - 1), -(2 ** 31))
    hi = max(min(hi, 2 ** 31 - 1), -(2 ** 31))
    return lo, hi


def _threshold(mask_matrix, target_matrix, threshold_range, preserve, honour_flags):
    if mask_matrix.dtype != np.uint8 or mask_matrix.ndim != 3:
        raise TypeError("mask matrix must be a 3-D uint8 array")
    if target_matrix.dtype != np.int16 or target_matrix.ndim != 3:
        raise TypeError("image matrix must be a 3-D int16 array")
    if tuple(mask_matrix.shape) != tuple(s + 1 for s in target_matrix.shape):
        raise ValueError("mask matrix must be image shape + 1 per axis (invesalius/data/mask.py:422-431)")
    lo, hi = _int_bounds(threshold_range)
    L.check(L.lib().ivx_threshold_all_slices(
        L.ptr(target_matrix), L.i64(target_matrix.shape), L.i64(target_matrix.strides), ctypes.c_int(lo),
        ctypes.c_int(hi), ctypes.c_int(int(preserve)), ctypes.c_int(int(honour_flags)), L.ptr(mask_matrix),
        L.i64(mask_matrix.strides)), "do_threshold_to_all_slices")
    if hasattr(mask_matrix, "flush"):
        mask_matrix.flush()  # slice_.py:1769


def do_threshold_to_all_slices(mask_matrix, target_matrix, threshold_range):
    """Slice.do_threshold_to_all_slices (invesalius/data/slice_.py:1739-1769) with do_threshold_to_a_slice
    (:1722-1737) fused: slices whose flag ``mask_matrix[n,0,0]`` is 0 get ``255*in_range`` with existing
    1/2/253/254 preserved, and their flag set to 1; flagged slices are left untouched."""
    _threshold(mask_matrix, target_matrix, threshold_range, True, True)


def set_mask_threshold(mask_matrix, image_matrix, threshold_range):
    """Whole-volume branch of Slice.SetMaskThreshold (invesalius/data/slice_.py:1240-1247): no preserve rule,
    every slice written, every flag forced to 1."""
    _threshold(mask_matrix, image_matrix, threshold_range, False, False)


def do_threshold_to_a_slice(slice_matrix: np.ndarray, mask: np.ndarray, threshold) -> np.ndarray:
    """Slice.do_threshold_to_a_slice (invesalius/data/slice_.py:1722-1737): returns a NEW uint8 array with
    255*in_range and the existing 1/2/253/254 of `mask` preserved.  2-D (or any-D) int16 slice, same-shape uint8 mask."""
    if slice_matrix.dtype != np.int16 or mask.dtype != np.uint8 or slice_matrix.shape != mask.shape:
        raise TypeError("slice must be int16 and mask a uint8 array of the same shape")
    out = np.array(mask, dtype=np.uint8, copy=True)
    img3 = slice_matrix.reshape((1, -1, slice_matrix.shape[-1])) if slice_matrix.ndim != 3 else slice_matrix
    m3 = out.reshape(img3.shape)
    # full-matrix layout expected by the C entry point: one flag row / column in front of every axis
    big = np.zeros(tuple(s + 1 for s in img3.shape), np.uint8)
    big[1:, 1:, 1:] = m3
    _threshold(big, np.ascontiguousarray(img3), threshold, True, False)
    return big[1:, 1:, 1:].reshape(slice_matrix.shape).copy()


def set_mask_threshold_slice(slice_: np.ndarray, threshold_range) -> np.ndarray:
    """Per-slice preview branch of Slice.SetMaskThreshold (slice_.py:1253-1256):
    ``(255 * ((slice_ >= thresh_min) & (slice_ <= thresh_max))).astype("uint8")``."""
    return do_threshold_to_a_slice(slice_, np.zeros(slice_.shape, np.uint8), threshold_range)


def project(slab: np.ndarray, axis: int, projection: int) -> np.ndarray:
    """MaxIP / MinIP / MeanIP of a slab: ``np.array(tmp_array).max|min|mean(axis)``
    (invesalius/data/slice_.py:885-889, 969-973, 1056-1060)."""
    if slab.ndim != 3:
        raise TypeError("slab must be 3-D")
    code = L.dtype_code(slab, (L.U8, L.I16, L.U16))
    op = {PROJECTION_MaxIP: L.MIP_MAX, PROJECTION_MinIP: L.MIP_MIN, PROJECTION_MeanIP: L.MIP_MEAN}[projection]
    oshape = tuple(s for i, s in enumerate(slab.shape) if i != axis)
    out = np.empty(oshape, np.float64 if op == L.MIP_MEAN else slab.dtype)
    L.check(L.lib().ivx_mip_reduce(code, L.ptr(slab), L.i64(slab.shape), L.i64(slab.strides), int(axis), int(op),
                                   L.ptr(out), L.i64(out.strides)), "project")
    return out


PROJECTION_LMIP, PROJECTION_MIDA, PROJECTION_CONTOUR_MIP, PROJECTION_CONTOUR_LMIP, PROJECTION_CONTOUR_MIDA = 4, 5, 6, 7, 8
_AXIS = {"AXIAL": 0, "CORONAL": 1, "SAGITAL": 2}


def view_matrix(q_orientation, center) -> np.ndarray:
    """The 4x4 matrix ``Slice.get_image_slice`` builds for a reoriented view (invesalius/data/slice_.py:848-858):
    ``T1 . R^T . T0`` with ``T0 = translation(-cz, -cy, -cx)``, ``R = quaternion_matrix(q_orientation)`` (w, x, y, z;
    transformations.py:1261-1290, unit-normalised there, identity below 4 eps) and ``T1 = translation(cz, cy, cx)``;
    `center` is the reference's ``(cx, cy, cz)``.  C-contiguous float64, as apply_view_matrix_transform requires."""
    q = np.array(q_orientation, dtype=np.float64, copy=True)
    n = float(np.dot(q, q))
    R = np.identity(4)
    if n >= np.finfo(float).eps * 4.0:
        q *= np.sqrt(2.0 / n)
        o = np.outer(q, q)
        R = np.array([[1.0 - o[2, 2] - o[3, 3], o[1, 2] - o[3, 0], o[1, 3] + o[2, 0], 0.0],
                      [o[1, 2] + o[3, 0], 1.0 - o[1, 1] - o[3, 3], o[2, 3] - o[1, 0], 0.0],
                      [o[1, 3] - o[2, 0], o[2, 3] + o[1, 0], 1.0 - o[1, 1] - o[2, 2], 0.0],
                      [0.0, 0.0, 0.0, 1.0]])
    cx, cy, cz = (float(v) for v in center)
    T0, T1 = np.identity(4), np.identity(4)
    T0[:3, 3] = (-cz, -cy, -cx)
    T1[:3, 3] = (cz, cy, cx)
    M = np.identity(4)
    for m in (T1, R.T, T0):  # transformations.concatenate_matrices: left to right
        M = np.dot(M, m)
    return np.ascontiguousarray(M)


def get_image_slice(matrix: np.ndarray, orientation: str, slice_number: int, number_slices: int = 1, inverted: bool = False,
                    border_size: float = 1.0, type_projection: int = PROJECTION_NORMAL, window_level=0, q_orientation=None,
                    center=None, spacing=None, interp_method: int = 2) -> np.ndarray:
    """The array work of ``Slice.get_image_slice`` (invesalius/data/slice_.py:832-1119): the slab
    ``matrix[n : n + number_slices]`` along the view axis (one slice for PROJECTION_NORMAL); when the view is reoriented
    (``np.any(q_orientation[1:])``, :847,862,948,1035) the slab is resampled from the whole volume through
    `view_matrix(q_orientation, center)` with ``apply_view_matrix_transform(matrix, spacing, M, n, orientation,
    interp_method, matrix.min(), slab)`` (HIP: csrc/k_transform.hip) before anything else; then reversed when `inverted`,
    then the projection -- max / min / mean, MIDA, the three contour MIPs -- with the reference's own arguments, its quirk
    included (the window LEVEL goes in for level and width alike: :898-900,906-945).  LMIP raises AttributeError like the
    reference (`mips.lmip` is commented out of invesalius_rs/__init__.py:83).  The buffer_slices cache stays with the
    caller; `interp_method` defaults to the reference's (Slice.interp_method = 2, slice_.py:119)."""
    from . import invesalius_rs as mips

    ax = _AXIS[orientation]
    if type_projection == PROJECTION_NORMAL:
        number_slices = 1
    sl = [slice(None)] * 3
    sl[ax] = slice(slice_number, slice_number + number_slices)
    tmp = np.array(matrix[tuple(sl)])
    if q_orientation is not None and np.any(np.asarray(q_orientation)[1:]):
        if center is None or spacing is None:
            raise TypeError("a reoriented view needs `center` (cx, cy, cz) and `spacing`")
        mips.apply_view_matrix_transform(matrix, spacing, view_matrix(q_orientation, center), slice_number, orientation,
                                         interp_method, matrix.min(), tmp)
    oshape = tuple(s for i, s in enumerate(tmp.shape) if i != ax)
    if type_projection == PROJECTION_NORMAL:
        return tmp.reshape(oshape)
    if inverted:
        rev = [slice(None)] * 3
        rev[ax] = slice(None, None, -1)
        tmp = tmp[tuple(rev)]
    if type_projection in (PROJECTION_MaxIP, PROJECTION_MinIP, PROJECTION_MeanIP):
        return project(tmp, ax, type_projection)
    if type_projection == PROJECTION_LMIP:
        raise AttributeError("module 'invesalius_rs' has no attribute 'lmip'")
    out = np.empty(oshape, tmp.dtype)
    if type_projection == PROJECTION_MIDA:
        mips.mida(tmp, ax, int(window_level), int(window_level), out)
    elif type_projection in (PROJECTION_CONTOUR_MIP, PROJECTION_CONTOUR_LMIP, PROJECTION_CONTOUR_MIDA):
        mips.fast_countour_mip(tmp, border_size, ax, window_level, window_level, type_projection - PROJECTION_CONTOUR_MIP, out)
    else:  # (:946-947: anything else shows the plain slice)
        sl[ax] = slice_number
        return np.array(matrix[tuple(sl)])
    return out


def apply_reorientation(matrix: np.ndarray, spacing, q_orientation, center, interp_method: int = 2, masks=()):
    """The array work of ``Slice.apply_reorientation`` (invesalius/data/slice_.py:1969-2068): bake the view's rotation into
    the data.  `matrix` (the int16 image, e.g. the ``matrix.dat`` memmap) is resampled IN PLACE from a copy of itself
    through ``M = view_matrix(q_orientation, center)`` -- ``apply_view_matrix_transform(copy, spacing, M, 0, "AXIAL",
    interp_method, copy.min(), matrix)`` (:1979-1988; HIP: csrc/k_transform.hip) -- and flushed.  Then every mask of `masks`
    (objects with ``.matrix``, the padded ``(dz+1, dy+1, dx+1)`` uint8 array, and ``.was_edited``): an edited mask goes
    through the SAME call with nearest-neighbour interpolation and cval 0 (:2034-2043) -- on the whole padded matrix, flag
    planes included, exactly as the reference does (its voxel (z, y, x) sits at matrix index (z+1, y+1, x+1), so the mask
    turns about a point one voxel off the image's: a reference quirk, kept) -- a threshold mask is cleared (:2055-2062);
    ``mask.clear_history()`` is called where it exists.  Returns the view state the reference leaves behind:
    ``(q_orientation, center) = ((1, 0, 0, 0), [s * d / 2 for d, s in zip(shape[::-1], spacing)])`` (:2002-2003)."""
    from . import invesalius_rs as mips

    if matrix.ndim != 3:
        raise TypeError("matrix must be a 3-D array")
    M = view_matrix(q_orientation, center)
    mcopy = np.array(matrix)  # (the reference's temporary memmap copy)
    mips.apply_view_matrix_transform(mcopy, spacing, M, 0, "AXIAL", int(interp_method), mcopy.min(), matrix)
    del mcopy
    if hasattr(matrix, "flush"):
        matrix.flush()
    new_mask_shape = tuple(s + 1 for s in matrix.shape)
    for mask in masks:
        mm = mask.matrix
        if tuple(mm.shape) != new_mask_shape:  # (:2028-2030 would recreate it; the image's shape never changes here)
            raise ValueError("mask matrix must be image shape + 1 per axis (invesalius/data/mask.py:422-431)")
        if getattr(mask, "was_edited", False):
            mask_copy = np.array(mm)
            mips.apply_view_matrix_transform(mask_copy, spacing, M, 0, "AXIAL", 0, 0, mm)
            del mask_copy
        else:
            mm[:] = 0
            resident.touch(mm)
        if hasattr(mm, "flush"):
            mm.flush()
        if hasattr(mask, "clear_history"):
            mask.clear_history()
    return np.array((1, 0, 0, 0)), [(s * d / 2.0) for (d, s) in zip(matrix.shape[::-1], spacing)]


def calc_image_area(mask_matrix: np.ndarray, spacing) -> float:
    """Slice.calc_image_area (invesalius/data/slice_.py:2296-2322) after its threshold step: the exposed-face area of
    ``mask_matrix[1:,1:,1:] > 127`` for ``spacing = (sx, sy, sz)``.  Computed from the uint8 mask on the GPU (the
    reference builds ``bin_img * 1.0`` and calls convolve_non_zero(..., cval=1).sum()); per-voxel terms are identical,
    the final sum is a tree sum instead of numpy's pairwise one (differs by rounding only)."""
    if mask_matrix.dtype != np.uint8 or mask_matrix.ndim != 3:
        raise TypeError("mask matrix must be a 3-D uint8 array")
    inner = mask_matrix[1:, 1:, 1:]
    sp = (ctypes.c_double * 3)(*[float(v) for v in spacing])
    area = ctypes.c_double(0.0)
    L.check(L.lib().ivx_mask_area(L.ptr(inner), L.i64(inner.shape), L.i64(inner.strides), sp, ctypes.byref(area)), "mask_area")
    return float(area.value)


BOOLEAN_UNION, BOOLEAN_DIFF, BOOLEAN_AND, BOOLEAN_XOR = 1, 2, 3, 4  # invesalius/constants.py:818-821


def do_boolean_op(op: int, m1_matrix: np.ndarray, m2_matrix: np.ndarray) -> np.ndarray:
    """Slice.do_boolean_op (slice_.py:1878-1923), the array part: a new padded mask matrix filled with 1 (flags
    "thresholded"), interior = 255 where op(m1 > 2, m2 > 2).  Both inputs are padded (dz+1, dy+1, dx+1) matrices that
    the caller has brought up to date (the reference calls do_threshold_to_all_slices on both first)."""
    if m1_matrix.shape != m2_matrix.shape or m1_matrix.dtype != np.uint8 or m2_matrix.dtype != np.uint8:
        raise TypeError("two uint8 mask matrices of the same shape")
    if op not in (BOOLEAN_UNION, BOOLEAN_DIFF, BOOLEAN_AND, BOOLEAN_XOR):
        raise ValueError("unknown boolean operation %r" % (op,))
    out = np.ones(m1_matrix.shape, np.uint8)
    a, b, m = m1_matrix[1:, 1:, 1:], m2_matrix[1:, 1:, 1:], out[1:, 1:, 1:]
    L.check(L.lib().ivx_mask_boolean(int(op), L.ptr(a), L.i64(a.strides), L.ptr(b), L.i64(b.strides), L.ptr(m),
                                     L.i64(m.strides), L.i64(m.shape)), "mask_boolean")
    return out


def calc_image_density(image: np.ndarray, mask_matrix: np.ndarray):
    """Slice.calc_image_density (slice_.py:2284-2297): (min, max, mean, std) of ``image[mask[1:,1:,1:] > 127]``, or
    four zeros when the mask selects nothing.  min / max are exact.  The device returns count, sum and sum of squares as
    exact integers; the mean is one float64 division (== np.mean), the variance is the exact rational
    ``(cnt * s2 - s1**2) / cnt**2`` rounded to float64 once, and std is its square root: within 2 ulp of the true value,
    also where every selected voxel is (nearly) the same -- sqrt(E[x^2] - mean^2) formed in float64 cancels there and was
    off by 3e-6 .. 7e-4 relative.  The sums cross the host interface as doubles, so they are exact below 2^53 only: more
    than about 8 M selected voxels all at +-32767 are out of that range."""
    if image.dtype != np.int16 or image.ndim != 3:
        raise TypeError("image must be a 3-D int16 array")
    inner = mask_matrix[1:, 1:, 1:]
    if inner.shape != image.shape or mask_matrix.dtype != np.uint8:
        raise TypeError("mask matrix must be uint8 and one voxel larger than the image on every axis")
    out = np.zeros(5, np.float64)
    L.check(L.lib().ivx_masked_density_i16(L.ptr(image), L.i64(image.strides), L.ptr(inner), L.i64(inner.strides),
                                           L.i64(image.shape), L.ptr(out)), "masked_density")
    cnt, s1, s2 = (int(v) for v in out[:3])
    lo, hi = out[3:]
    if cnt == 0:
        return 0, 0, 0, 0
    mean = s1 / cnt
    var = float(Fraction(cnt * s2 - s1 * s1, cnt * cnt))
    return int(lo), int(hi), float(mean), math.sqrt(var)


_FILTER_PLANES = {"Axial": 0, "Coronal": 1, "Sagittal": 2}  # _run_filter's axis_map (slice_.py:2384)


def apply_image_filter(matrix: np.ndarray, filter_type: int, value, dimension: str = "3D", orientation: str = "Axial"):
    """The compute part of Slice.__apply_image_filter / _run_filter (slice_.py:2330-2430): filter type 0 Gaussian,
    1 median, 2 mean, 3 sharpen, 4 despeckle, 5 border detection (filters.py) over the whole volume, or with
    ``dimension != "3D"`` slice by slice along the orientation's axis (Axial 0, Coronal 1, Sagittal 2; anything else 0)
    -- in one library call, not one per slice.  Returns ``result.astype(matrix.dtype)`` as the reference stashes it;
    an unknown filter type returns None (the reference returns without a result)."""
    from . import filters

    if filter_type not in filters.FILTER_NAMES:
        return None
    if dimension == "3D":
        plane = -1
    else:
        if getattr(matrix, "ndim", 0) != 3:
            raise TypeError("the 2D mode filters the slices of a 3-D image")
        plane = _FILTER_PLANES.get(orientation, 0)
    if filter_type == filters.MEDIAN:
        filters.median_size(value)
    elif filter_type == filters.MEAN:
        filters.mean_size(value)
    result = filters.image_filter(matrix, filter_type, value, plane)
    return result.astype(matrix.dtype)


# ---- the manual edition panel -------------------------------------------------------------------------------------
BRUSH_DRAW, BRUSH_ERASE, BRUSH_THRESH, BRUSH_THRESH_ERASE, BRUSH_THRESH_ADD_ONLY, BRUSH_THRESH_ERASE_ONLY = range(6)  # constants.py:341-346
BRUSH_FILL = 6  # IVX_BRUSH_FILL: the marker brush and the generic brush write a given byte


def _axis(orientation: str) -> int:
    try:
        return _AXIS[orientation]
    except KeyError:
        raise ValueError("orientation must be AXIAL, CORONAL or SAGITAL") from None


def _slice_views(mask_matrix, image_matrix, orientation, n):
    """(mask slice view, flag cell view, image slice view) of Slice.get_mask_slice (slice_.py:1142-1173)"""
    ax = _axis(orientation)
    n = int(n)
    if mask_matrix.dtype != np.uint8 or mask_matrix.ndim != 3:
        raise TypeError("mask matrix must be a 3-D uint8 array")
    if not 0 <= n < mask_matrix.shape[ax] - 1:
        raise IndexError("slice %d outside the volume" % n)
    m = [slice(1, None)] * 3
    m[ax] = n + 1
    f = [slice(0, 1)] * 3
    f[ax] = slice(n + 1, n + 2)
    image = None
    if image_matrix is not None:
        if image_matrix.dtype != np.int16 or tuple(mask_matrix.shape) != tuple(s + 1 for s in image_matrix.shape):
            raise TypeError("image must be int16 and the mask matrix one voxel larger on every axis (invesalius/data/mask.py:422-431)")
        i = [slice(None)] * 3
        i[ax] = n
        image = image_matrix[tuple(i)]
    return mask_matrix[tuple(m)], mask_matrix[tuple(f)], image


def get_mask_slice(mask_matrix, image_matrix, orientation: str, n: int, threshold_range) -> np.ndarray:
    """Slice.get_mask_slice (invesalius/data/slice_.py:1121-1175), the lazy threshold of one slice in any orientation: when
    the slice's flag cell -- ``[n+1,0,0]`` AXIAL, ``[0,n+1,0]`` CORONAL, ``[0,0,n+1]`` SAGITAL -- is 0, the slice
    ``matrix[n+1, 1:, 1:]`` (and siblings) is thresholded with the preserve rule and the flag set to 1, in place; returns
    a copy of the slice.  (The buffer_slices cache in front of it stays with the caller.)"""
    mview = _thresholded_slice_view(mask_matrix, image_matrix, orientation, n, threshold_range)
    return np.array(mview, dtype=mask_matrix.dtype)


def _thresholded_slice_view(mask_matrix, image_matrix, orientation, n, threshold_range):
    """the lazy threshold of get_mask_slice; returns the slice as a view of the matrix"""
    mview, flag, _ = _slice_views(mask_matrix, image_matrix, orientation, n)
    if flag.reshape(-1)[0] == 0:
        if threshold_range is None:
            raise ValueError("slice %d (%s) has not been thresholded yet (its flag is 0): pass the mask's threshold_range" % (n, orientation))
        ax = _axis(orientation)
        order = (ax,) + tuple(a for a in range(3) if a != ax)  # the slice's axis in front: one "axial" slice of a strided volume
        mt, it = mask_matrix.transpose(order), image_matrix.transpose(order)
        lo, hi = _int_bounds(threshold_range)
        img1, m2 = it[n:n + 1], mt[n:n + 2]
        L.check(L.lib().ivx_threshold_all_slices(L.ptr(img1), L.i64(img1.shape), L.i64(img1.strides), ctypes.c_int(lo), ctypes.c_int(hi),
                                                 ctypes.c_int(1), ctypes.c_int(1), L.ptr(m2), L.i64(m2.strides)), "get_mask_slice")
    return mview


def _op_runs(operations, ndabs):
    """maximal runs of one operation: [(operation, dabs)]"""
    if not hasattr(operations, "__iter__"):
        return [(int(operations), ndabs)] if ndabs else []
    ops = [int(o) for o in operations]
    if len(ops) != ndabs:
        raise ValueError("one operation per position")
    runs = []
    for o in ops:
        if runs and runs[-1][0] == o:
            runs[-1][1] += 1
        else:
            runs.append([o, 1])
    return [(o, k) for o, k in runs]


def _brush_stroke(matrix, image_matrix, orientation, n, index, positions, operations, thresh=(0, 0), fill_value=0, padded=True,
                  set_flag=False, want_previous=False):
    """ivx_mask_brush_stroke: the dabs of `positions` under the footprint `index`, in runs of one operation, on slice `n`"""
    from . import cursor

    ax = _axis(orientation)
    if np.ndim(index) != 2:
        raise TypeError("the footprint is a 2-D array")
    index = np.ascontiguousarray(np.asarray(index) != 0).view(np.uint8)
    if matrix.dtype != np.uint8 or matrix.ndim != 3:
        raise TypeError("the matrix must be a 3-D uint8 array")
    ishape = tuple(s - 1 for s in matrix.shape) if padded else tuple(matrix.shape)
    h, w = (ishape[a] for a in range(3) if a != ax)
    positions = list(positions)
    dabs = np.ascontiguousarray(cursor.dab_windows(positions, index.shape, w))
    runs = _op_runs(operations, len(positions))
    reads = any(BRUSH_THRESH <= o <= BRUSH_THRESH_ERASE_ONLY for o, _ in runs)
    if reads and (image_matrix is None or image_matrix.dtype != np.int16 or tuple(image_matrix.shape) != ishape):
        raise TypeError("the threshold operations need the int16 image the mask belongs to")
    lo, hi = _int_bounds(thresh)
    run_ops = (ctypes.c_int32 * max(len(runs), 1))(*[o for o, _ in runs])
    run_lens = (L.c_i64 * max(len(runs), 1))(*[k for _, k in runs])
    previous = np.empty((h, w), np.uint8) if want_previous else None
    L.check(L.lib().ivx_mask_brush_stroke(
        L.ptr(matrix), L.i64(ishape), L.i64(matrix.strides), L.ptr(image_matrix) if reads else None,
        L.i64(image_matrix.strides) if reads else None, ctypes.c_int(ax), L.c_i64(int(n)), L.ptr(index), L.c_i64(index.shape[0]),
        L.c_i64(index.shape[1]), L.ptr(dabs), run_ops, run_lens, L.c_i64(len(runs)), ctypes.c_int(lo), ctypes.c_int(hi),
        ctypes.c_int(int(fill_value) & 255), ctypes.c_int(int(padded)), ctypes.c_int(int(set_flag)),
        L.ptr(previous) if want_previous else None), "brush_stroke")
    return previous


def edit_mask_stroke(mask_matrix, image_matrix, orientation: str, n: int, index, positions, operations=BRUSH_THRESH,
                     edition_threshold_range=(0, 0), threshold_range=None, set_flag: bool = True, return_previous: bool = False):
    """A whole drag of the brush on slice `n`: Slice.edit_mask_pixel (invesalius/data/slice_.py:656-744) for every position,
    then the write-back and flag of Slice.apply_slice_buffer_to_mask (:1925-1967) -- on the GPU, in place on the padded mask
    matrix, staging the slice alone.  `index` is the footprint (cursor.cursor_pixels), `positions` the slice
    pixels the cursor visited -- ``(px, py)`` pairs, floats allowed, or flat integers -- `operations` one BRUSH_* value or
    one per position (the modifier keys can change during a drag: the stroke is split into maximal runs of one operation,
    launched in order).  The slice is first brought up to date with `threshold_range` (the mask's own), as the reference's
    viewer has done before any brush event (get_mask_slice); the range may be left out only for a slice whose flag says it
    is up to date already.  Returns the slice as it was before the stroke (p_mask, what `history.EditionHistory.new_node` takes as the state before) when
    asked."""
    if threshold_range is not None:
        get_mask_slice(mask_matrix, image_matrix, orientation, n, threshold_range)
    elif _slice_views(mask_matrix, image_matrix, orientation, n)[1].reshape(-1)[0] == 0:
        raise ValueError("slice %d (%s) has not been thresholded yet (its flag is 0): pass the mask's threshold_range" % (n, orientation))
    return _brush_stroke(mask_matrix, image_matrix, orientation, n, index, positions, operations, edition_threshold_range,
                         padded=True, set_flag=set_flag, want_previous=return_previous)


def edit_mask_pixel(mask_matrix, image_matrix, orientation: str, n: int, operation: int, index, position,
                    edition_threshold_range=(0, 0), threshold_range=None, set_flag: bool = True, return_previous: bool = False):
    """One dab: Slice.edit_mask_pixel (slice_.py:656-744) -- `edit_mask_stroke` with a single position."""
    return edit_mask_stroke(mask_matrix, image_matrix, orientation, n, index, [position], operation, edition_threshold_range,
                            threshold_range, set_flag, return_previous)


def apply_slice_buffer_to_mask(mask_matrix, orientation: str, n: int, b_mask) -> np.ndarray:
    """Slice.apply_slice_buffer_to_mask (slice_.py:1925-1967) for callers that keep the reference's buffer-slice flow: the
    caller's edited slice goes into the matrix, the slice's flag becomes 2; returns the previous slice (p_mask).  The slice
    travels through a device block, so that a bound matrix gets exactly these bytes in its mirror (a `touch` of a coronal or
    sagittal view would upload nearly the whole matrix again)."""
    from .device import DeviceBuffer

    mview, flag, _ = _slice_views(mask_matrix, None, orientation, n)
    b = np.ascontiguousarray(b_mask, dtype=np.uint8)
    if b.shape != mview.shape:
        raise ValueError("the buffer slice has shape %r, the mask's slice %r" % (b.shape, mview.shape))
    p_mask = mview.copy()
    buf = DeviceBuffer(b.size + 16)
    try:
        buf.upload(np.concatenate([b.reshape(-1), np.array([2], np.uint8)]))
        buf.download_view(mview)
        L.check(L.lib().ivx_download_strided(L.ptr(flag), L.i64((1, 1, 1)), L.i64((1, 1, 1)), buf.at(b.size), 1), "apply_slice_buffer")
    finally:
        buf.close()
    return p_mask


# ---- the image geometry tools ---------------------------------------------------------------------------------------
def _volume(a, what):
    if not isinstance(a, np.ndarray) or a.ndim != 3 or a.itemsize not in (1, 2, 4, 8):
        raise TypeError("%s: a 3-D array with items of 1, 2, 4 or 8 bytes" % what)
    return a


def _versions(versions, matrix):
    """the other image versions (Project.image_versions: arrays, or (label, array) pairs), without `matrix` itself"""
    mats = [v[1] if isinstance(v, tuple) else v for v in versions]
    return [m for m in mats if m is not matrix]


def _mask_matrix(mask) -> np.ndarray:
    return mask.matrix if hasattr(mask, "matrix") else mask


def _clear_mask(mask):
    """``mask.matrix[:] = 0`` (slice_.py:2136-2146), flag planes included: zeros on the host and, for a bound matrix, a
    device memset of its mirror -- the mask crosses the link in neither direction"""
    mm = _mask_matrix(mask)
    if mm.flags["C_CONTIGUOUS"] and mm.size:
        L.check(L.lib().ivx_host_zero(L.ptr(mm), mm.nbytes), "clear mask")
    else:
        mm[...] = 0
        resident.touch(mm)
    if hasattr(mm, "flush"):
        mm.flush()
    if hasattr(mask, "clear_history"):
        mask.clear_history()


def flip_volume(matrix: np.ndarray, axis: int, masks=(), versions=()):
    """The array work of ``Slice.OnFlipVolume`` (invesalius/data/slice_.py:2103-2149), in place: ``matrix[:] = matrix[::-1]``
    on `axis` 0 / 1 / 2 of the (z, y, x) matrix, the same for every other image version of `versions` (arrays, or the
    (label, array) pairs of ``Project.image_versions``), then every mask of `masks` (objects with ``.matrix``, or the padded
    matrices themselves) zeroed whole, flag planes included, so that the lazy per-slice threshold evaluates it again.  A
    bound image (`bind_image`) is flipped in its mirror and written to the host once; its binding stays valid."""
    if axis not in (0, 1, 2):
        raise ValueError("axis must be 0, 1 or 2")
    for m in [matrix] + _versions(versions, matrix):
        _volume(m, "flip_volume")
        L.check(L.lib().ivx_image_flip(L.ptr(m), L.i64(m.shape), L.i64(m.strides), m.itemsize, int(axis)), "flip_volume")
        if hasattr(m, "flush"):
            m.flush()
    for mask in masks:
        _clear_mask(mask)


def swapped_spacing(spacing, axes):
    """``spacing`` (sx, sy, sz) after the matrix axes `axes` changed places (slice_.py:2184-2189; the reference spells out
    the three pairs its menu sends, (2, 1), (2, 0) and (1, 0) -- the same pair in the other order means the same here)"""
    a, b = (int(v) for v in axes)
    sp = list(spacing)
    sp[2 - a], sp[2 - b] = sp[2 - b], sp[2 - a]
    return tuple(sp)


def _swapped(m, a, b, bound):
    new_shape = list(m.shape)
    new_shape[a], new_shape[b] = new_shape[b], new_shape[a]
    new = np.empty(new_shape, m.dtype)
    new.fill(0)  # (written by the host first: a download into pages nobody has touched faults them in one by one, 190 against 35 ms at 512^3)
    if bound and new.size:
        resident.bind_zeros(new, keep=True)  # (the call below writes the host array and this mirror: no upload)
    L.check(L.lib().ivx_image_swap_axes(L.ptr(m), L.i64(m.shape), L.i64(m.strides), m.itemsize, a, b, L.ptr(new), L.i64(new.strides)),
            "swap_volume_axes")
    return new


def _release_binding(a):
    r = resident.find(a)
    if r is not None and r.array is resident._root(a):
        r.release()


def swap_volume_axes(matrix: np.ndarray, axes, spacing, masks=(), versions=()):
    """The array work of ``Slice.OnSwapVolumeAxes`` (invesalius/data/slice_.py:2151-2251): returns ``(new_matrix,
    new_spacing, new_mask_matrices, new_versions)`` with ``new_matrix = np.array(matrix.swapaxes(*axes))``, the spacing
    permuted (`swapped_spacing`), every other image version swapped alike and every mask a matrix of zeros of the new shape
    + 1 (set on the mask object where `masks` holds objects with ``.matrix``).  What was bound stays bound: the new arrays
    are registered with a mirror the swap itself fills, the old bindings are released; no image byte goes to the device.
    The package holds the new bindings until ``resident.find(array).release()``.  The reference's memmap file replacement
    stays with the caller."""
    a, b = (int(v) for v in axes)
    if a == b or not {a, b} <= {0, 1, 2}:
        raise ValueError("axes must be two different ones of 0, 1, 2")
    _volume(matrix, "swap_volume_axes")
    others = _versions(versions, matrix)
    new_matrix = None
    new_versions = []
    for m in [matrix] + others:
        _volume(m, "swap_volume_axes")
        bound = resident.find(m) is not None
        new = _swapped(m, a, b, bound)
        if bound:
            _release_binding(m)
        if m is matrix:
            new_matrix = new
        else:
            new_versions.append(new)
    new_mask_shape = tuple(s + 1 for s in new_matrix.shape)
    new_masks = []
    for mask in masks:
        mm = _mask_matrix(mask)
        if tuple(mm.shape) != new_mask_shape:  # Mask._recreate_mask_matrix (:2237-2239)
            bound = resident.find(mm) is not None
            new = np.zeros(new_mask_shape, mm.dtype)
            if bound:
                _release_binding(mm)
                resident.bind_zeros(new, keep=True)
            if hasattr(mask, "matrix"):
                mask.matrix = new
            if hasattr(mask, "clear_history"):
                mask.clear_history()
        else:
            _clear_mask(mask)
            new = mm
        new_masks.append(new)
    return new_matrix, swapped_spacing(spacing, (a, b)), new_masks, new_versions


def gantry_tilt_shifts(depth: int, spacing, tilt) -> np.ndarray:
    """the first component of the shift FixGantryTilt hands scipy for slice n (imagedata_utils.py:148-154), in its own
    order of operations: ``-(tan(radians(tilt)) * n * spacing[2]) / spacing[1]``"""
    gntan = math.tan(np.radians(tilt))
    out = np.empty(int(depth), np.float64)
    for n in range(int(depth)):
        offset = gntan * n * spacing[2]
        out[n] = -offset / spacing[1]
    return out


def fix_gantry_tilt(matrix: np.ndarray, spacing, tilt, masks=()):
    """``imagedata_utils.FixGantryTilt(matrix, spacing, tilt)`` (invesalius/data/imagedata_utils.py:143-154), in place and
    bit for bit: slice n becomes ``scipy.ndimage.shift(slice, (shift_n, 0), cval=matrix.min())`` -- cubic spline, mode
    "constant", int16 -- with the minimum taken anew before every slice (HIP: csrc/k_imagegeo.hip; the arithmetic is
    csrc/imagegeo_math.h).  A bound image is corrected in its mirror and written to the host once.  The reference runs this
    at import, before any mask exists; masks handed in `masks` are cleared like a flip clears them.  Returns the fill value
    every slice was given."""
    if not isinstance(matrix, np.ndarray) or matrix.dtype != np.int16 or matrix.ndim != 3:
        raise TypeError("matrix must be a 3-D int16 array")
    shifts = gantry_tilt_shifts(matrix.shape[0], spacing, tilt)
    cvals = np.zeros(matrix.shape[0], np.int32)
    L.check(L.lib().ivx_image_fix_gantry_tilt(L.ptr(matrix), L.i64(matrix.shape), L.i64(matrix.strides), L.ptr(shifts), L.ptr(cvals)),
            "fix_gantry_tilt")
    if hasattr(matrix, "flush"):
        matrix.flush()
    for mask in masks:
        _clear_mask(mask)
    return cvals


# ---- the slice display ------------------------------------------------------------------------------------------------
def _plane(a, orientation, n):
    sl = [slice(None)] * 3
    sl[_axis(orientation)] = int(n)
    return a[tuple(sl)]


def get_aux_slice(aux_matrix: np.ndarray, orientation: str, n: int) -> np.ndarray:
    """Slice.get_aux_slice (invesalius/data/slice_.py:1177-1184): slice `n` of an aux matrix (of the image's shape)"""
    return np.array(_plane(aux_matrix, orientation, n))


def _picture(a, what, channels):
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != channels:
        raise TypeError("%s: a (h, w, %d) uint8 array" % (what, channels))
    return a if a.strides[2] == 1 else np.ascontiguousarray(a)


def _image_kind(image, what):
    from . import slice_display as D

    if not isinstance(image, np.ndarray) or image.ndim != 2 or image.dtype not in (np.dtype(np.int16), np.dtype(np.float64)):
        raise TypeError("%s: a 2-D int16 (or, for MeanIP, float64) array" % what)
    return D.IMG_I16 if image.dtype == np.int16 else D.IMG_F64


def do_ww_wl(image: np.ndarray, state) -> np.ndarray:
    """Slice.do_ww_wl (slice_.py:1656-1695) on a 2-D int16 / float64 slice: the (h, w, 3) picture of rule R1 (grey), R3 (PLIST)
    or R4 (WIDGET)."""
    from . import slice_display as D

    p, blob = D.build(state, _image_kind(image, "do_ww_wl"), D.ST_WWWL)
    return D.run(p, blob, image, None, None, *image.shape)


def do_colour_image(imagedata: np.ndarray, state, image_range) -> np.ndarray:
    """Slice.do_colour_image (slice_.py:1771-1795) on do_ww_wl's picture: the identity in the PLIST and WIDGET modes, else the
    HSV table of rule R2 indexed by the first channel; `image_range` is the whole image's (min, max)."""
    from . import slice_display as D

    imagedata = _picture(imagedata, "do_colour_image", 3)
    if state.from_ in (D.PLIST, D.WIDGET):
        return imagedata
    p, blob = D.build(state, D.IMG_U8, D.ST_COLOUR, image_range=image_range)
    return D.run(p, blob, imagedata[:, :, 0], None, None, *imagedata.shape[:2])


def do_colour_mask(mask_slice: np.ndarray, state) -> np.ndarray:
    """Slice.do_colour_mask (slice_.py:1797-1827): the (h, w, 4) RGBA overlay of rule R5 for a 2-D uint8 mask slice"""
    from . import slice_display as D

    if mask_slice.dtype != np.uint8 or mask_slice.ndim != 2:
        raise TypeError("do_colour_mask: a 2-D uint8 array")
    p, blob = D.build(state, D.IMG_U8, D.ST_MASK, have_mask=True, out_channels=4)
    return D.run(p, blob, None, mask_slice, None, *mask_slice.shape)


def do_custom_colour(aux_slice: np.ndarray, map_colours: dict) -> np.ndarray:
    """Slice.do_custom_colour (slice_.py:1829-1859): the (h, w, 4) RGBA overlay of rule R6; the smallest key must be 0"""
    from . import slice_display as D

    if aux_slice.dtype != np.uint8 or aux_slice.ndim != 2:
        raise TypeError("do_custom_colour: a 2-D uint8 array")
    p, blob = D.build(D.DisplayState(), D.IMG_U8, D.ST_AUX, aux_colours=map_colours, out_channels=4)
    return D.run(p, blob, None, None, aux_slice, *aux_slice.shape)


def do_blend(imagedata: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """Slice.do_blend (slice_.py:1861-1873): the RGBA overlay over the RGB picture at opacity 0.8, rule R7"""
    from . import slice_display as D

    imagedata, mask = _picture(imagedata, "do_blend", 3), _picture(mask, "do_blend", 4)
    if imagedata.shape[:2] != mask.shape[:2]:
        raise ValueError("do_blend: picture %r, overlay %r" % (imagedata.shape, mask.shape))
    p, blob = D.build(D.DisplayState(), D.IMG_RGB8, D.ST_BLEND)
    return D.run(p, blob, imagedata, mask, None, *imagedata.shape[:2])


def get_slices(image_matrix, mask_matrix, orientation: str, slice_number: int, number_slices: int, state, inverted: bool = False,
               border_size: float = 1.0, type_projection: int = PROJECTION_NORMAL, threshold_range=None, aux_matrix=None,
               q_orientation=None, center=None, spacing=None, interp_method: int = 2, image_range=None) -> np.ndarray:
    """``Slice.GetSlices`` (invesalius/data/slice_.py:746-830) without its buffer_slices cache: the final (h, w, 3) uint8
    picture of slice `slice_number` -- window/level, colour table, the current mask's overlay (`mask_matrix`, the padded
    matrix, or None; drawn when ``state.mask_shown``), then the aux overlay ``state.to_show_aux`` over `aux_matrix` -- from one
    kernel launch (csrc/k_slice_show.hip; the rules are DESIGN 7l).  `state` is a slice_display.DisplayState.  A plain slice of
    a bound image and mask crosses the link once, as the picture; a projection or a reoriented view is computed by
    `get_image_slice` first (MIDA and the contour MIPs get ``state.window_level`` like in the reference).  A mask slice whose
    flag is 0 is thresholded in place with `threshold_range` first, exactly like `get_mask_slice`.  `image_range`, the whole
    image's (min, max) that the colour table's range needs, is taken with numpy per call like the reference does unless
    given."""
    from . import slice_display as D

    reoriented = q_orientation is not None and bool(np.any(np.asarray(q_orientation)[1:]))
    if type_projection == PROJECTION_NORMAL and not reoriented:
        if not 0 <= int(slice_number) < image_matrix.shape[_axis(orientation)]:
            raise IndexError("slice %d outside the volume" % slice_number)
        image = _plane(image_matrix, orientation, slice_number)  # a view: a bound image is read from its mirror
    else:
        image = get_image_slice(image_matrix, orientation, slice_number, number_slices, inverted, border_size, type_projection,
                                state.window_level, q_orientation, center, spacing, interp_method)
    kind = _image_kind(image, "get_slices")
    mask = None
    if mask_matrix is not None and state.mask_shown:
        mask = _thresholded_slice_view(mask_matrix, image_matrix, orientation, slice_number, threshold_range)
    aux, aux_colours = None, D.aux_colour_dict(state, mask_matrix is not None)
    if aux_colours is not None:
        if aux_matrix is None or aux_matrix.dtype != np.uint8 or tuple(aux_matrix.shape) != tuple(image_matrix.shape):
            raise TypeError("the aux overlay %r needs its uint8 matrix of the image's shape" % state.to_show_aux)
        aux = _plane(aux_matrix, orientation, slice_number)
    if state.from_ == D.OTHER and image_range is None:
        image_range = (image_matrix.min(), image_matrix.max())
    p, blob = D.build(state, kind, D.ST_ALL, image_range=image_range, have_mask=mask is not None, aux_colours=aux_colours)
    return D.run(p, blob, image, mask, aux, *image.shape)
