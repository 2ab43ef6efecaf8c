"""The display state of ``invesalius.data.slice_.Slice`` and the byte tables of the slice display.

``Slice.GetSlices`` (invesalius/data/slice_.py:746-830) reads window/level, the colour mode and the mask's colour from the
``Slice`` singleton; here that state is a plain `DisplayState` handed to ``slice_.get_slices``.  The tables the kernel indexes
(csrc/k_slice_show.hip) are built here, in Python only: rule R2 is *defined* through Python's ``colorsys.hsv_to_rgb``, so the
builder calls the definition itself instead of restating it in C, and the tables are 3 KB made once per state, not per pixel.
The per-pixel arithmetic (R1, the indices of R2 / R3 / R6, R4's interpolation, R7) is csrc/slice_show_math.h.
"""
from __future__ import annotations

import colorsys
import ctypes
import functools
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L

OTHER, PLIST, WIDGET = 0, 1, 2  # invesalius/data/slice_.py:58-60
ST_WWWL, ST_COLOUR, ST_MASK, ST_AUX, ST_BLEND = 1, 2, 4, 8, 16  # IVX_SHOW_*: the reference's five seams
ST_ALL = 31
IMG_I16, IMG_F64, IMG_U8, IMG_RGB8 = 0, 1, 2, 3
MAX_NODES = 256

# const.SLICE_COLOR_TABLE (invesalius/constants.py:187-197): name -> (number of colours, saturation range, hue range, value range)
SLICE_COLOR_TABLE = {
    "Default ": (None, (0, 0), (0, 0), (0, 1)),
    "Hue": (None, (1, 1), (0, 1), (1, 1)),
    "Saturation": (None, (0, 1), (0.6, 0.6), (1, 1)),
    "Desert": (256, (1, 1), (0, 0.1), (1, 1)),
    "Rainbow": (256, (1, 1), (0, 0.8), (1, 1)),
    "Ocean": (256, (1, 1), (0.667, 0.5), (1, 1)),
    "Inverse Gray": (256, (0, 0), (0, 0), (1, 0)),
}
THRESHOLD_HUE_RANGE = (0, 0.6667)  # constants.py:287
MASK_OPACITY = 0.40                # constants.py:293
MASK_COLOUR = [[0.33, 1, 0.33], [1, 1, 0.33], [0.33, 0.91, 1], [1, 0.33, 1], [1, 0.68, 0.33], [1, 0.33, 0.33],
               [0.33333333333333331, 0.33333333333333331, 1.0], [0.74901960784313726, 1.0, 0.0],
               [0.83529411764705885, 0.33333333333333331, 1.0]]  # constants.py:295-306
# the two colour dicts GetSlices itself holds (slice_.py:809-813, :822-827)
AUX_WATERSHED = {0: (0.0, 0.0, 0.0, 0.0), 1: (0.0, 1.0, 0.0, 1.0), 2: (1.0, 0.0, 0.0, 1.0)}
AUX_DEFAULT = {0: (0.0, 0.0, 0.0, 0.0), 1: (0.0, 0.0, 0.0, 0.0), 254: (1.0, 0.0, 0.0, 1.0), 255: (1.0, 0.0, 0.0, 1.0)}


@dataclass
class Node:
    """gui/widgets/clut_imagedata.py:29-31: ordered by value alone"""
    value: float
    colour: tuple = field(compare=False)

    def __lt__(self, other):
        return self.value < other.value


@dataclass
class DisplayState:
    """What GetSlices reads from the Slice singleton and the current mask (slice_.py:97-119)."""
    window_width: float = 255.0
    window_level: float = 127.0
    from_: int = OTHER
    saturation_range: tuple = (0, 0)
    hue_range: tuple = (0, 0)
    value_range: tuple = (0, 1)
    values: object = None          # PLIST: the (r, g, b) triples of presets.get_wwwl_preset_colours
    nodes: object = None           # WIDGET: Node objects, or (value, (r, g, b)) pairs
    mask_colour: tuple = tuple(MASK_COLOUR[0])
    opacity: float = MASK_OPACITY
    mask_shown: bool = True
    to_show_aux: str = ""
    aux_colours: dict = field(default_factory=dict)  # Slice.aux_matrices_colours

    def set_colour_table(self, name: str):
        """Slice.UpdateColourTableBackground(const.SLICE_COLOR_TABLE[name]) (slice_.py:1515-1523)"""
        _, self.saturation_range, self.hue_range, self.value_range = SLICE_COLOR_TABLE[name]
        self.from_ = OTHER

    def set_plist(self, values):
        """Slice.UpdateColourTableBackgroundPlist (slice_.py:1525-1531)"""
        self.values = [tuple(int(c) for c in v) for v in np.asarray(values).reshape(-1, 3)]
        self.from_ = PLIST

    def set_widget_nodes(self, nodes):
        """Slice.UpdateColourTableBackgroundWidget (slice_.py:1533-1555): the window follows the nodes"""
        self.nodes = _nodes(nodes)
        self.from_ = WIDGET
        self.window_width, self.window_level = window_level_from_nodes(self.nodes)


def _nodes(nodes):
    return [n if isinstance(n, Node) else Node(float(n[0]), tuple(int(c) for c in n[1])) for n in nodes]


def window_level_from_nodes(nodes):
    """(window width, window level) of UpdateColourTableBackgroundWidget (slice_.py:1548-1553)"""
    knodes = sorted(_nodes(nodes))
    p0, pn = knodes[0].value, knodes[-1].value
    return pn - p0, (pn + p0) / 2


def update_wwwl_widget_nodes(nodes, ww, wl):
    """Slice._update_wwwl_widget_nodes (slice_.py:1697-1720), in place on `nodes` (Node objects): the nodes follow a
    window / level drag -- shifted to the new level, spread about the middle to the new width."""
    knodes = sorted(nodes)
    p1, p2 = knodes[0], knodes[-1]
    half = (p2.value - p1.value) / 2.0
    middle = p1.value + half
    shift_wl = wl - middle
    shift_ww = p1.value + shift_wl - (wl - 0.5 * ww)
    for n, node in enumerate(knodes):
        factor = max(abs(node.value - middle) / half, 0)
        node.value += shift_wl
        if n < len(nodes) / 2.0:
            node.value -= shift_ww * factor
        else:
            node.value += shift_ww * factor
    return nodes


def table_range(image_min, image_max, ww, wl):
    """(tmin, tmax) of do_colour_image (slice_.py:1776-1780): ``iu.get_LUT_value_255(np.array((min, max)), ww, wl)``
    (imagedata_utils.py:540-552) with its own order of operations; the array keeps the dtype of (min, max), so an int16
    image's range is truncated to integers like numpy's piecewise does."""
    data = np.array((image_min, image_max))
    out = np.empty(2, data.dtype)
    for k, d in enumerate(data):
        if d <= (wl - 0.5 - (ww - 1) / 2):
            out[k] = 0
        elif d > (wl - 0.5 + (ww - 1) / 2):
            out[k] = 255
        else:
            out[k] = np.array(((d - (wl - 0.5)) / (ww - 1) + 0.5) * 255).astype(data.dtype)
    return float(out[0]), float(out[1])


def _byte(c) -> int:
    return int(c * 255 + 0.5)


def _frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)  # (the builders below are memoized: a drag or a scroll asks for the same table every picture)
    return a


def _pair(r):
    return float(r[0]), float(r[1])


def hsv_table(saturation_range, hue_range, value_range) -> np.ndarray:
    """R2: 256 RGBA entries, entry i from ``colorsys.hsv_to_rgb`` at x0 + i * ((x1 - x0) / 255) of each range (read-only)"""
    return _hsv_table(_pair(saturation_range), _pair(hue_range), _pair(value_range))


@functools.lru_cache(maxsize=32)
def _hsv_table(saturation_range, hue_range, value_range):
    out = np.zeros((256, 4), np.uint8)
    steps = [(r[0], (r[1] - r[0]) / 255) for r in (hue_range, saturation_range, value_range)]
    for i in range(256):
        h, s, v = (x0 + i * dx for x0, dx in steps)
        out[i, :3] = [_byte(c) for c in colorsys.hsv_to_rgb(h, s, v)]
        out[i, 3] = 255
    return _frozen(out)


def plist_table(values) -> np.ndarray:
    """R3: the plist's colours, the grey ramp beyond them (read-only)"""
    return _plist_table(tuple(tuple(int(c) for c in v) for v in list(values)[:256]))


@functools.lru_cache(maxsize=32)
def _plist_table(values):
    out = np.zeros((256, 4), np.uint8)
    for i in range(256):
        out[i, :3] = values[i] if i < len(values) else (_byte(i / 255),) * 3
        out[i, 3] = 255
    return _frozen(out)


def mask_table(colour, opacity) -> np.ndarray:
    """R5: entries 253 .. 255 the mask's colour at its opacity, everything else transparent (read-only)"""
    return _mask_table(tuple(float(c) for c in tuple(colour)[:3]), float(opacity))


@functools.lru_cache(maxsize=32)
def _mask_table(colour, opacity):
    out = np.zeros((256, 4), np.uint8)
    r, g, b = colour
    out[253:256] = (_byte(r), _byte(g), _byte(b), _byte(opacity))
    return _frozen(out)


def custom_table(map_colours):
    """R6: (256 RGBA entries, largest key); keys not in the dict are transparent (read-only)"""
    return _custom_table(tuple(sorted((int(k), tuple(float(c) for c in rgba)) for k, rgba in map_colours.items())))


@functools.lru_cache(maxsize=32)
def _custom_table(items):
    keys = [k for k, _ in items]
    if not keys or min(keys) != 0:
        raise ValueError("the smallest key of a custom colour table must be 0 (the reference indexes the table by the key itself)")
    if max(keys) > 255:
        raise ValueError("custom colour keys are uint8 values")
    out = np.zeros((256, 4), np.uint8)
    for k, rgba in items:
        out[k] = [_byte(c) for c in rgba]
    return _frozen(out), max(keys)


def aux_colour_dict(state: DisplayState, have_mask: bool):
    """the colour dict GetSlices hands do_custom_colour (slice_.py:800-829), or None when no aux overlay is drawn"""
    if state.to_show_aux == "watershed" and have_mask and state.mask_shown:
        return AUX_WATERSHED
    if state.to_show_aux and have_mask:
        return state.aux_colours.get(state.to_show_aux, AUX_DEFAULT)
    return None


class Params(ctypes.Structure):
    """struct ivx_slice_show_params (include/ivx.h)"""
    _fields_ = [("image_kind", ctypes.c_int32), ("mode", ctypes.c_int32), ("stages", ctypes.c_int32), ("n_nodes", ctypes.c_int32),
                ("aux_max", ctypes.c_int32), ("out_channels", ctypes.c_int32), ("window_width", ctypes.c_double),
                ("window_level", ctypes.c_double), ("table_min", ctypes.c_double), ("table_max", ctypes.c_double)]


def pack_tables(image_table=None, mask_tab=None, aux_tab=None, nodes=()) -> np.ndarray:
    """the kernel's tables block: 3 x 256 RGBA, then the sorted nodes' values and their colours / 255 as float64"""
    nodes = sorted(_nodes(nodes))
    if len(nodes) > MAX_NODES:
        raise ValueError("at most %d widget nodes" % MAX_NODES)
    blob = np.zeros(3072 + 32 * len(nodes), np.uint8)
    for k, t in enumerate((image_table, mask_tab, aux_tab)):
        if t is not None:
            blob[1024 * k:1024 * (k + 1)] = np.asarray(t, np.uint8).reshape(1024)
    d = blob[3072:].view(np.float64)
    d[:len(nodes)] = [n.value for n in nodes]
    d[len(nodes):] = [c / 255.0 for n in nodes for c in n.colour]
    return blob


def build(state: DisplayState, image_kind: int, stages: int, image_range=None, have_mask: bool = False, aux_colours=None,
          out_channels: int = 3):
    """(Params, tables block) of one picture.  `image_range` (min, max of the whole image) is needed by R2 alone."""
    ww, wl = float(state.window_width), float(state.window_level)
    if (stages & ST_WWWL) and not ww > 0:
        raise ValueError("window width must be positive")
    image_table, tmin, tmax, nodes = None, 0.0, 0.0, ()
    if state.from_ == PLIST:
        if stages & ST_WWWL:
            image_table = plist_table(state.values)
    elif state.from_ == WIDGET:
        if stages & ST_WWWL:
            nodes = state.nodes
            if not nodes:
                raise ValueError("the widget mode needs nodes")
    elif stages & ST_COLOUR:
        if image_range is None:
            raise ValueError("the colour table's range needs the image's (min, max)")
        image_table = hsv_table(state.saturation_range, state.hue_range, state.value_range)
        tmin, tmax = table_range(image_range[0], image_range[1], ww, wl)
    mask_tab = mask_table(state.mask_colour, state.opacity) if (stages & ST_MASK) and have_mask else None
    aux_tab, aux_max = None, 0
    if (stages & ST_AUX) and aux_colours is not None:
        aux_tab, aux_max = custom_table(aux_colours)
    blob = pack_tables(image_table, mask_tab, aux_tab, nodes)
    p = Params(int(image_kind), int(state.from_), int(stages), len(nodes), int(aux_max), int(out_channels), ww, wl, tmin, tmax)
    return p, blob


def _view2(a, item):
    """(pointer, row stride, element stride) of a 2-D view (or a (h, w, k) picture with dense pixels)"""
    if a is None:
        return None, 0, 0
    if a.ndim == 3 and (a.strides[2] != a.itemsize or a.itemsize != 1):
        raise TypeError("a picture's channels must be dense bytes")
    return L.ptr(a), int(a.strides[0]), int(a.strides[1])


def run(params: Params, blob: np.ndarray, image, mask, aux, h: int, w: int) -> np.ndarray:
    """ivx_slice_show on host arrays (views of bound arrays are served from their mirrors)"""
    out = np.empty((h, w, params.out_channels), np.uint8)
    ip, irs, ies = _view2(image, None)
    mp, mrs, mes = _view2(mask, None)
    ap, ars, aes = _view2(aux, None)
    c = L.c_i64
    L.check(L.lib().ivx_slice_show(ip, c(irs), c(ies), mp, c(mrs), c(mes), ap, c(ars), c(aes), c(h), c(w), ctypes.byref(params),
                                   L.ptr(blob), L.ptr(out)), "slice_show")
    return out
