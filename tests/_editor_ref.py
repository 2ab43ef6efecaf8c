"""numpy restatement of the slice editing tools, line for line after the reference -- Slice.edit_mask_pixel,
get_mask_slice, apply_slice_buffer_to_mask (invesalius/data/slice_.py:656-744, 1121-1175, 1925-1967), the two style brushes
(styles.py:392-461, 2000-2069), do_2d_seg (:3082-3149), CropMask (:2654-2694), the two _calculate_area_pixels
(cursor_actors.py:302-330, 377-395).  tests/test_editor_host.py holds it against tests/golden/ref_editor.npz bit for bit; the GPU
tests use it where the fixture has no case.  Everything acts in place on the arrays it is given, like the reference."""
import math

import numpy as np

ORIENTATIONS = ("AXIAL", "CORONAL", "SAGITAL")
DRAW, ERASE, THRESH, THRESH_ERASE, THRESH_ADD_ONLY, THRESH_ERASE_ONLY = range(6)


def slice_of(a, orientation, n):
    return a[n] if orientation == "AXIAL" else (a[:, n, :] if orientation == "CORONAL" else a[:, :, n])


def flag_index(orientation, n):
    return {"AXIAL": (n + 1, 0, 0), "CORONAL": (0, n + 1, 0), "SAGITAL": (0, 0, n + 1)}[orientation]


def cursor_pixels(fmt, radius, unit, spacing, orientation):
    r = radius
    if unit == "µm":
        r /= 1000.0
    if fmt == "circle":
        if unit == "px":
            sx, sy = 1.0, 1.0
        else:
            sx, sy = {"AXIAL": (spacing[0], spacing[1]), "CORONAL": (spacing[0], spacing[2]), "SAGITAL": (spacing[1], spacing[2])}[orientation]
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
    return np.ones((y, x), dtype="bool")


def window(index, position, width):
    """(xi, xf, yi, yf) before the clips (slice_.py:661-695)"""
    if hasattr(position, "__iter__"):
        px, py = position
    else:
        py = position / width
        px = position % width
    cx = index.shape[1] / 2 + 1
    cy = index.shape[0] / 2 + 1
    xi = int(px - index.shape[1] + cx)
    xf = int(xi + index.shape[1])
    yi = int(py - index.shape[0] + cy)
    yf = int(yi + index.shape[0])
    return xi, xf, yi, yf


def _clipped(index, position, shape):
    xi, xf, yi, yf = window(index, position, shape[1])
    if yi < 0:
        index = index[abs(yi):, :]
        yi = 0
    if yf > shape[0]:
        index = index[: index.shape[0] - (yf - shape[0]), :]
        yf = shape[0]
    if xi < 0:
        index = index[:, abs(xi):]
        xi = 0
    if xf > shape[1]:
        index = index[:, : index.shape[1] - (xf - shape[1])]
        xf = shape[1]
    if (not 0 <= xi <= shape[1] and not 0 <= xf <= shape[1]) or (not 0 <= yi <= shape[0] and not 0 <= yf <= shape[0]):
        return None
    return index, xi, xf, yi, yf


def edit_mask_pixel(mask, image, operation, index, position, edition_threshold_range):
    """one dab on the 2-D buffer slice `mask` (slice_.py:656-744).  Where the reference raises -- the two *_ONLY operations with a
    window that ends left of or above the slice (negative xf / yf, :733, :735) -- nothing was written: a no-op here."""
    thresh_min, thresh_max = edition_threshold_range
    c = _clipped(index, position, image.shape)
    if c is None:
        return
    index, xi, xf, yi, yf = c
    roi_m = mask[yi:yf, xi:xf]
    roi_i = image[yi:yf, xi:xf]
    if roi_i.size:
        if operation == THRESH:
            roi_m[index] = (((roi_i[index] >= thresh_min) & (roi_i[index] <= thresh_max)) * 253) + 1
        elif operation == THRESH_ERASE:
            roi_m[index] = (((roi_i[index] < thresh_min) | (roi_i[index] > thresh_max)) * 253) + 1
        elif operation in (THRESH_ADD_ONLY, THRESH_ERASE_ONLY):
            if index.shape != roi_i.shape:
                return
            if operation == THRESH_ADD_ONLY:
                roi_m[((index) & (roi_i >= thresh_min) & (roi_i <= thresh_max))] = 254
            else:
                roi_m[((index) & ((roi_i < thresh_min) | (roi_i > thresh_max)))] = 1
        elif operation == DRAW:
            roi_m[index] = 254
        elif operation == ERASE:
            roi_m[index] = 1


def fill_pixel(matrix2d, fill_value, index, position):
    """the marker brush / the generic brush on a 2-D slice view (styles.py:392-461, 2000-2069)"""
    c = _clipped(index, position, matrix2d.shape)
    if c is None:
        return
    index, xi, xf, yi, yf = c
    roi_m = matrix2d[yi:yf, xi:xf]
    if roi_m.size:
        roi_m[index] = fill_value


def do_threshold_to_a_slice(slice_matrix, mask, threshold):
    thresh_min, thresh_max = threshold
    m = ((slice_matrix >= thresh_min) & (slice_matrix <= thresh_max)) * 255
    m[mask == 1] = 1
    m[mask == 2] = 2
    m[mask == 253] = 253
    m[mask == 254] = 254
    return m.astype("uint8")


def get_mask_slice(matrix, image, orientation, n, threshold_range):
    f = flag_index(orientation, n)
    view = slice_of(matrix[1:, 1:, 1:], orientation, n)
    if matrix[f] == 0:
        view[:] = do_threshold_to_a_slice(slice_of(image, orientation, n), view, threshold_range)
        matrix[f] = 1
    return np.array(view)


def apply_slice_buffer_to_mask(matrix, orientation, n, b_mask):
    view = slice_of(matrix[1:, 1:, 1:], orientation, n)
    p_mask = view.copy()
    view[:] = b_mask
    matrix[flag_index(orientation, n)] = 2
    return p_mask


def stroke(matrix, image, orientation, n, index, positions, operations, edition_threshold_range, threshold_range):
    """a drag as the reference plays it: get_mask_slice, one edit_mask_pixel per position on the buffer slice, then
    apply_slice_buffer_to_mask; returns p_mask"""
    b = get_mask_slice(matrix, image, orientation, n, threshold_range)
    ops = operations if hasattr(operations, "__iter__") else [operations] * len(positions)
    for op, pos in zip(ops, positions):
        edit_mask_pixel(b, slice_of(image, orientation, n), op, index, pos, edition_threshold_range)
    return apply_slice_buffer_to_mask(matrix, orientation, n, b)


def do_threshold_to_all_slices(matrix, image, threshold_range):
    for n in range(1, matrix.shape[0]):
        if matrix[n, 0, 0] == 0:
            m = matrix[n, 1:, 1:]
            m[:] = do_threshold_to_a_slice(image[n - 1], m, threshold_range)
            matrix[n, 0, 0] = 1


def crop_mask(matrix, image, limits, threshold_range):
    xi, xf, yi, yf, zi, zf = (v + 1 for v in limits)
    do_threshold_to_all_slices(matrix, image, threshold_range)
    tmp = matrix[zi - 1: zf + 1, yi - 1: yf + 1, xi - 1: xf + 1].copy()
    matrix[:] = 1
    matrix[zi - 1: zf + 1, yi - 1: yf + 1, xi - 1: xf + 1] = tmp


def get_lut_value_255(data, window, level):
    shape = data.shape
    data_ = data.ravel()
    data = np.piecewise(data_, [data_ <= (level - 0.5 - (window - 1) / 2), data_ > (level - 0.5 + (window - 1) / 2)],
                        [0, 255, lambda d: ((d - (level - 0.5)) / (window - 1) + 0.5) * (255)])
    data.shape = shape
    return data


def floodfill_threshold(data, seeds, t0, t1, fill, strct, out):
    """invesalius_rs floodfill_threshold (floodfill.rs:96-170) behind its wrapper's int() of the bounds (__init__.py:32-35)"""
    t0, t1 = int(t0), int(t1)
    dz, dy, dx = data.shape
    oz, oy, ox = (s // 2 for s in strct.shape)
    stack = []
    for (i, j, k) in seeds:
        if t0 <= data[k, j, i] <= t1:
            stack.append((i, j, k))
            out[k, j, i] = fill
    offs = [(kk - oz, jj - oy, ii - ox) for kk in range(strct.shape[0]) for jj in range(strct.shape[1]) for ii in range(strct.shape[2])
            if strct[kk, jj, ii]]
    while stack:
        x, y, z = stack.pop()
        out[z, y, x] = fill
        for a, b, c in offs:
            zo, yo, xo = z + a, y + b, x + c
            if 0 <= zo < dz and 0 <= yo < dy and 0 <= xo < dx and out[zo, yo, xo] != fill and t0 <= data[zo, yo, xo] <= t1:
                out[zo, yo, xo] = fill
                stack.append((xo, yo, zo))


def _structure2(con_2d):
    g = np.indices((3, 3)) - 1
    return (np.abs(g).sum(axis=0) <= {4: 1, 8: 2}[con_2d]).astype("uint8").reshape((1, 3, 3))


def do_2d_seg(matrix, image3, seed_xy, orientation, n, method, con_2d, fill_value, t0=None, t1=None, dev_min=0, dev_max=0,
              use_ww_wl=False, ww=None, wl=None, confid_mult=2.5, confid_iters=3):
    """styles.py:3082-3149 with do_rg_confidence (:3220-3251); False when the click is rejected"""
    x, y = seed_xy
    view = slice_of(matrix[1:, 1:, 1:], orientation, n)
    mask = view.copy()
    image = slice_of(image3, orientation, n)
    bstruct = _structure2(con_2d)
    dy, dx = image.shape
    if method == "confidence":
        image = image.reshape((1, dy, dx))
        if use_ww_wl:
            image = get_lut_value_255(image, ww, wl)
        bool_mask = np.zeros((1, dy, dx), dtype="bool")
        out_mask = np.zeros((1, dy, dx), np.uint8)
        bool_mask[0, max(y - 1, 0): y + 2, max(x - 1, 0): x + 2] = True
        for _ in range(confid_iters):
            var = np.std(image[bool_mask])
            mean = np.mean(image[bool_mask])
            floodfill_threshold(image, ((x, y, 0),), mean - var * confid_mult, mean + var * confid_mult, 1, bstruct, out_mask)
            bool_mask[out_mask == 1] = True
    else:
        if method == "dynamic":
            if use_ww_wl:
                image = get_lut_value_255(image, ww, wl)
            v = image[y, x]
            t0 = v - dev_min
            t1 = v + dev_max
        if image[y, x] < t0 or image[y, x] > t1:
            return False
        image = image.reshape((1, dy, dx))
        out_mask = np.zeros((1, dy, dx), np.uint8)
        floodfill_threshold(image, ((x, y, 0),), t0, t1, 1, bstruct, out_mask)
    mask[out_mask[0].astype("bool")] = fill_value
    view[:] = mask
    return True
