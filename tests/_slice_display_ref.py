"""The maintainers' statement of the slice display, rules R1 - R7 of DESIGN 7l, in numpy and Python numbers (float64).

VTK is not available to this project: what vtkImageMapToWindowLevelColors, vtkLookupTable, vtkWindowLevelLookupTable,
vtkColorTransferFunction, vtkImageMapToColors and vtkImageBlend compute is PARITY UNPINNED.  This file is the definition the
kernel (csrc/k_slice_show.hip, csrc/slice_show_math.h) is held to, bit for bit.  It shares no code with the product.
"""
import colorsys

import numpy as np

OTHER, PLIST, WIDGET = 0, 1, 2


def u8(x):
    """truncation of a non-negative double to uint8"""
    x = np.asarray(x, np.float64)
    assert (x >= 0).all() and (x < 256).all()
    return np.floor(x).astype(np.uint8)


def byte(c):
    return int(float(c) * 255 + 0.5)


# ---- R1 -----------------------------------------------------------------------------------------------------------------------------
def ww_wl_grey(v, ww, wl):
    if not ww > 0:
        raise ValueError("window width must be positive")
    ww, wl = float(ww), float(wl)
    v = np.asarray(v)
    f_lo = wl - ww / 2
    f_hi = f_lo + ww
    if v.dtype == np.int16:
        lo_c, hi_c = min(max(f_lo, -32768.0), 32767.0), min(max(f_hi, -32768.0), 32767.0)
        lo, hi = float(int(lo_c)), float(int(hi_c))
    else:
        assert v.dtype == np.float64
        lo_c, hi_c = f_lo, f_hi
        lo, hi = lo_c, hi_c
    lo_val = int(min(max(255 * (lo_c - f_lo) / ww, 0.0), 255.0))
    hi_val = int(min(max(255 * (hi_c - f_lo) / ww, 0.0), 255.0))
    x = v.astype(np.float64)
    shift, scale = ww / 2 - wl, 255 / ww
    mid = (x + shift) * scale
    inside = (x > lo) & (x < hi)
    g = np.where(x <= lo, lo_val, hi_val).astype(np.uint8)
    g[inside] = u8(mid[inside])
    return g


# ---- R2 -----------------------------------------------------------------------------------------------------------------------------
def hsv_table(saturation_range, hue_range, value_range, n=256):
    t = np.zeros((n, 4), np.uint8)
    for i in range(n):
        h, s, v = (float(r[0]) + i * ((float(r[1]) - float(r[0])) / (n - 1)) for r in (hue_range, saturation_range, value_range))
        t[i] = [byte(c) for c in colorsys.hsv_to_rgb(h, s, v)] + [255]
    return t


def lut_value_255(d, ww, wl):
    """iu.get_LUT_value_255 of one number, its own order of operations"""
    if d <= (wl - 0.5 - (ww - 1) / 2):
        return 0
    if d > (wl - 0.5 + (ww - 1) / 2):
        return 255
    return ((d - (wl - 0.5)) / (ww - 1) + 0.5) * 255


def table_range(image_min, image_max, ww, wl):
    """the reference hands get_LUT_value_255 ``np.array((min, max))``: np.piecewise keeps that dtype, so an int16 image's
    range is truncated toward zero"""
    dt = np.array((image_min, image_max)).dtype
    return tuple(float(np.array(lut_value_255(d, ww, wl)).astype(dt)) for d in (image_min, image_max))


def colour_index(g, tmin, tmax, n=256):
    g = np.asarray(g).astype(np.float64)
    if tmax <= tmin:
        return np.where(g > tmin, n - 1, 0)
    return np.clip(np.trunc((g - tmin) * (n / (tmax - tmin))), 0, n - 1).astype(np.int64)


def colour_image(g, table, tmin, tmax):
    return table[colour_index(g, tmin, tmax)][..., :3]


# ---- R3 -----------------------------------------------------------------------------------------------------------------------------
def plist_table(values):
    t = np.zeros((256, 4), np.uint8)
    for i in range(256):
        t[i, :3] = values[i] if i < len(values) else (byte(i / 255),) * 3
        t[i, 3] = 255
    return t


def plist_index(v, ww, wl):
    v = np.asarray(v).astype(np.float64)
    return np.clip(np.trunc((v - (wl - ww / 2)) * (256 / ww)), 0, 255).astype(np.int64)


# ---- R4 -----------------------------------------------------------------------------------------------------------------------------
def widget_colour(v, nodes):
    """nodes: (value, (r, g, b)) pairs; sorted here by value (stable)"""
    nodes = sorted(nodes, key=lambda n: n[0])
    xs = [float(n[0]) for n in nodes]
    v = np.asarray(v).astype(np.float64)
    out = np.zeros(v.shape + (3,), np.uint8)
    flat, o = v.reshape(-1), out.reshape(-1, 3)
    cache = {}
    for i, x in enumerate(flat):
        x = float(x)
        if x not in cache:
            k = -1
            for j, xn in enumerate(xs):
                if xn <= x:
                    k = j
            if k < 0:
                c = [byte(ch / 255) for ch in nodes[0][1]]
            elif k == len(nodes) - 1:
                c = [byte(ch / 255) for ch in nodes[-1][1]]
            else:
                t = (x - xs[k]) / (xs[k + 1] - xs[k])
                c = []
                for c0, c1 in zip(nodes[k][1], nodes[k + 1][1]):
                    c.append(int((c0 / 255 + (c1 / 255 - c0 / 255) * t) * 255 + 0.5))
            cache[x] = c
        o[i] = cache[x]
    return out


# ---- R5, R6 -------------------------------------------------------------------------------------------------------------------------
def mask_table(colour, opacity):
    t = np.zeros((256, 4), np.uint8)
    r, g, b = colour[:3]
    t[253:] = (byte(r), byte(g), byte(b), byte(opacity))
    return t


def colour_mask(m, colour, opacity):
    return mask_table(colour, opacity)[m]


def custom_colour(v, map_colours):
    if min(map_colours) != 0:
        raise ValueError("the smallest key must be 0")
    mx = max(map_colours)
    n = mx + 1
    t = np.zeros((n, 4), np.uint8)
    for k, rgba in map_colours.items():
        t[k] = [byte(c) for c in rgba]
    if mx == 0:
        return t[np.zeros(np.shape(v), np.int64)]
    idx = np.clip(np.trunc(np.asarray(v).astype(np.float64) * (n / mx)), 0, n - 1).astype(np.int64)
    return t[idx]


# ---- R7 -----------------------------------------------------------------------------------------------------------------------------
def blend(base, over):
    """base (.., 3) uint8, over (.., 4) uint8"""
    base, over = np.asarray(base).astype(np.int64), np.asarray(over).astype(np.int64)
    o = int(256 * 0.8 + 0.5)
    assert o == 205
    r = over[..., 3:4] * o
    f = 65280 - r
    return ((base * f + over[..., :3] * r) >> 16).astype(np.uint8)


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
def ww_wl(v, mode, ww, wl, values=None, nodes=None):
    """do_ww_wl: the RGB picture"""
    if mode == PLIST:
        return plist_table(values)[plist_index(v, ww, wl)][..., :3]
    if mode == WIDGET:
        return widget_colour(v, nodes)
    g = ww_wl_grey(v, ww, wl)
    return np.stack([g, g, g], -1)


def get_slices(image, mask, aux, *, mode=OTHER, ww, wl, ranges=((0, 0), (0, 0), (0, 1)), image_range=None, values=None, nodes=None,
               mask_colour=None, opacity=None, aux_colours=None):
    """image: the 2-D slice (get_image_slice's output); mask: get_mask_slice's output or None (not shown); aux: the aux
    slice or None; ranges: (saturation, hue, value)"""
    pic = ww_wl(image, mode, ww, wl, values, nodes)
    if mode == OTHER:
        tmin, tmax = table_range(image_range[0], image_range[1], ww, wl)
        pic = colour_image(pic[..., 0], hsv_table(*ranges), tmin, tmax)
    if mask is not None:
        pic = blend(pic, colour_mask(mask, mask_colour, opacity))
    if aux is not None:
        pic = blend(pic, custom_colour(aux, aux_colours))
    return np.ascontiguousarray(pic)
