"""The Image Filters dialog's six functions (invesalius/data/filters.py:5-66) on the GPU, same names and signatures.

The reference runs scipy.ndimage on the whole `Slice.matrix`; here every call is one `ivx_image_filter` (k_filter.hip),
bit for bit equal to scipy 1.15 for int16 images (2-D or 3-D, strided views included).  The result is a new array.
Only int16 is accepted (TypeError otherwise); there is no CPU fallback (RuntimeError without a device).

The Gaussian weights are computed here with numpy, exactly as scipy's `_gaussian_kernel1d` does: numpy's exp and libm's
need not agree in the last bit, and the int16 truncation after each pass turns such a bit into a different voxel.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L

GAUSSIAN, MEDIAN, MEAN, SHARPEN, DESPECKLE, BORDER = 0, 1, 2, 3, 4, 5  # the reference's filter_type (slice_.py:2370-2381)
FILTER_NAMES = {GAUSSIAN: "gaussian", MEDIAN: "median", MEAN: "mean", SHARPEN: "sharpen", DESPECKLE: "despeckle",
                BORDER: "sobel"}  # _after_filter's names for image_versions_meta (slice_.py:2470-2478)
MAX_RADIUS = 255  # IVX_FILTER_MAX_RADIUS


def gaussian_weights(sigma: float):
    """(w, r): scipy's gaussian_filter1d kernel for `sigma` (truncate 4.0) -- r = int(4 sigma + 0.5),
    w = exp(-0.5 / sigma^2 * x^2) / sum for x in -r..r -- or (None, -1) where gaussian_filter skips the axis (sigma <= 1e-15)."""
    sigma = float(sigma)
    if not sigma > 1e-15:
        return None, -1
    r = int(4.0 * sigma + 0.5)
    sigma2 = sigma * sigma
    x = np.arange(-r, r + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    return np.ascontiguousarray(phi_x, dtype=np.float64), r


def median_size(value: float) -> int:
    """filters.py:11: the window edge of median_blur_filter (3, 4 or 5)."""
    return max(3, min(int(2 * value + 1), 5))


def mean_size(value: float) -> int:
    """filters.py:17: the window edge of mean_blur_filter (<= 1: the identity)."""
    return int(2 * value + 1)


def _check(matrix) -> np.ndarray:
    if not isinstance(matrix, np.ndarray) or matrix.dtype != np.int16:
        raise TypeError("image filters take int16 arrays (got %s)" % getattr(matrix, "dtype", type(matrix).__name__))
    if matrix.ndim not in (2, 3):
        raise TypeError("image filters take 2-D or 3-D arrays (got %d-D)" % matrix.ndim)
    return matrix


def image_filter(matrix: np.ndarray, filter_type: int, value: float, plane_axis: int = -1, normalize: bool = True) -> np.ndarray:
    """One library call: filter `matrix` (int16, 2-D or 3-D) as the reference's filter `filter_type` with the dialog's
    `value`; `plane_axis` 0/1/2 filters every slice along that axis as a 2-D image (the "2D" mode of _run_filter)."""
    a = _check(matrix)
    filter_type = int(filter_type)
    if filter_type not in FILTER_NAMES:
        raise ValueError("unknown filter type %r" % (filter_type,))
    if a.ndim == 2 and plane_axis != -1:
        raise ValueError("a 2-D image has no slice axis")
    if plane_axis not in (-1, 0, 1, 2):
        raise ValueError("plane_axis must be -1, 0, 1 or 2")
    out = np.empty(a.shape, np.int16)
    if a.size == 0:
        return out
    L.require_device()
    if any(s < 0 for s in a.strides):
        a = np.ascontiguousarray(a)
    shape, st, ost = a.shape, a.strides, out.strides
    if a.ndim == 2:  # one slice of a (1, h, w) volume, filtered as a 2-D image
        shape, st, ost, plane_axis = (1,) + shape, (shape[0] * st[0],) + st, (out.nbytes,) + ost, 0
    sigma = 1.0 if filter_type == SHARPEN else value
    w, r = gaussian_weights(sigma) if filter_type in (GAUSSIAN, DESPECKLE, SHARPEN, BORDER) else (None, -1)
    if r > MAX_RADIUS:
        raise ValueError("sigma %r needs a kernel radius of %d (at most %d)" % (sigma, r, MAX_RADIUS))
    L.check(L.lib().ivx_image_filter(filter_type, ctypes.c_double(float(value)), int(plane_axis), int(bool(normalize)),
                                     None if w is None else L.ptr(w), int(r), L.I16, L.ptr(a), L.i64(shape), L.i64(st),
                                     L.ptr(out), L.i64(ost)), "image_filter")
    return out


def gaussian_blur_filter(matrix: np.ndarray, sigma: float) -> np.ndarray:
    return image_filter(matrix, GAUSSIAN, sigma)


def median_blur_filter(matrix: np.ndarray, value: float) -> np.ndarray:
    # Median Filter (3D, capped at size 5)
    median_size(value)  # the reference's int(): a NaN / infinite value raises as it does there
    return image_filter(matrix, MEDIAN, value)


def mean_blur_filter(matrix: np.ndarray, value: float) -> np.ndarray:
    # Mean Filter (fast separable 3D)
    mean_size(value)
    return image_filter(matrix, MEAN, value)


def sharpening_filter(matrix: np.ndarray, value: float) -> np.ndarray:
    # Sharpen via Unsharp Masking (sigma 1 blur, clipped to the image's range)
    return image_filter(matrix, SHARPEN, value)


def despeckle_filter(matrix: np.ndarray, value: float) -> np.ndarray:
    """Gaussian-based speckle reduction ('value' is the sigma)."""
    return image_filter(matrix, DESPECKLE, value)


def border_detection_filter(matrix: np.ndarray, value: float = 1.0, normalize: bool = True) -> np.ndarray:
    """Sobel gradient magnitude with Gaussian pre-smoothing of sigma 'value'; normalised to the image's range."""
    return image_filter(matrix, BORDER, value, normalize=normalize)
