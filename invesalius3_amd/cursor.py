"""The brush footprints of the manual edition panel and the window a dab covers.

`cursor_pixels` restates ``CursorCircle._calculate_area_pixels`` and ``CursorRectangle._calculate_area_pixels``
(invesalius/data/cursor_actors.py:302-330, 377-395) with their quirks; `dab_windows` is the host side of
csrc/slice_edit_math.h: the first column and row of a dab's unclipped window, which is what the stroke kernel takes."""
from __future__ import annotations

import math

import numpy as np

BRUSH_CIRCLE, BRUSH_SQUARE = 0, 1  # invesalius/constants.py:337-338
_FORMATS = {BRUSH_CIRCLE: "circle", BRUSH_SQUARE: "rectangle", "circle": "circle", "rectangle": "rectangle", "square": "rectangle"}


def cursor_pixels(format, radius, unit="mm", spacing=(1.0, 1.0, 1.0), orientation="AXIAL") -> np.ndarray:
    """The 2-D bool footprint of a brush: `format` BRUSH_CIRCLE / BRUSH_SQUARE (or "circle" / "rectangle").

    Kept from the reference: the unit "µm" divides the radius by 1000 and "px" uses spacing 1; the circle in SAGITAL
    orientation takes ``sx = spacing[1], sy = spacing[2]`` (the brush code pairs SAGITAL with spacing[2], spacing[1]); the
    rectangle is ``floor(2 r / s)`` wide in AXIAL but ``floor(r / s)`` in the other two orientations and can come out empty."""
    kind = _FORMATS[format]
    if orientation not in ("AXIAL", "CORONAL", "SAGITAL"):
        raise ValueError("orientation must be AXIAL, CORONAL or SAGITAL")
    r = radius
    if unit == "µm":
        r /= 1000.0
    if kind == "circle":
        if unit == "px":
            sx, sy = 1.0, 1.0
        elif orientation == "AXIAL":
            sx, sy = spacing[0], spacing[1]
        elif orientation == "CORONAL":
            sx, sy = spacing[0], spacing[2]
        else:
            sx, sy = spacing[1], spacing[2]
        xi, xf = math.floor(-r / sx), math.ceil(r / sx) + 1
        yi, yf = math.floor(-r / sy), math.ceil(r / sy) + 1
        y, x = np.ogrid[yi:yf, xi:xf]
        return (y * sy) ** 2 + (x * sx) ** 2 <= r ** 2
    sx, sy, sz = (1.0, 1.0, 1.0) if unit == "px" else spacing
    if orientation == "AXIAL":
        x, y = int(math.floor(2 * r / sx)), int(math.floor(2 * r / sy))
    elif orientation == "CORONAL":
        x, y = int(math.floor(r / sx)), int(math.floor(r / sz))
    else:
        x, y = int(math.floor(r / sy)), int(math.floor(r / sz))
    return np.ones((max(y, 0), max(x, 0)), dtype="bool")


def dab_windows(positions, index_shape, slice_width: int) -> np.ndarray:
    """(ndabs, 2) int32 of ``(xi, yi)``: where the footprint's unclipped window starts on the slice, for positions given as
    ``(px, py)`` pairs (floats allowed) or as flat integers (``py = position / W`` a float division, ``px = position % W``).
    The arithmetic is csrc/slice_edit_math.h, the text the kernel's bounds test is written in (host code: needs no device)."""
    import ctypes

    from . import _lib as L

    fh, fw = (int(v) for v in index_shape)
    lib = L.lib()
    xy = np.empty((len(positions), 2), np.float64)
    flat = (ctypes.c_double * 2)()
    for k, pos in enumerate(positions):
        if hasattr(pos, "__iter__"):
            xy[k] = pos
        else:
            L.check(lib.ivx_slice_flat_position(L.c_i64(int(pos)), L.c_i64(int(slice_width)), flat), "flat_position")
            xy[k] = flat[0], flat[1]
    out = np.empty((len(positions), 2), np.int32)
    L.check(lib.ivx_slice_dab_windows(L.ptr(xy), L.c_i64(len(positions)), L.c_i64(fh), L.c_i64(fw), L.ptr(out)), "dab_windows")
    return out


def dab_extent(window, index_shape, slice_shape, row_stride: int, elem_stride: int):
    """What the kernel's bounds test leaves of one dab: (footprint pixels inside the slice, lowest and highest byte offset
    they address in a view with these strides; both -1 when nothing is left).  csrc/slice_edit_math.h, on the host."""
    import ctypes

    from . import _lib as L

    out = (L.c_i64 * 3)()
    L.check(L.lib().ivx_slice_dab_extent(L.c_i64(int(window[0])), L.c_i64(int(window[1])), L.c_i64(int(index_shape[0])),
                                         L.c_i64(int(index_shape[1])), L.c_i64(int(slice_shape[0])), L.c_i64(int(slice_shape[1])),
                                         L.c_i64(int(row_stride)), L.c_i64(int(elem_stride)), out), "dab_extent")
    return int(out[0]), int(out[1]), int(out[2])


def dab_clip(window, index_shape, slice_shape):
    """The four clips of edit_mask_pixel (slice_.py:697-709) for one window: ``(xi, x_skip, x_count, yi, y_skip, y_count)`` --
    the clipped window starts at (xi, yi), `skip` footprint columns / rows are trimmed at the low side and `count` are left."""
    from . import _lib as L

    out = (L.c_i64 * 6)()
    L.check(L.lib().ivx_slice_dab_clip(L.c_i64(int(window[0])), L.c_i64(int(window[1])), L.c_i64(int(index_shape[0])),
                                       L.c_i64(int(index_shape[1])), L.c_i64(int(slice_shape[0])), L.c_i64(int(slice_shape[1])), out),
            "dab_clip")
    return tuple(int(v) for v in out)
