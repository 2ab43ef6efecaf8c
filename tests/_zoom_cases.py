"""Named cases for the order-2 zoom (csrc/k_zoom.hip = scipy.ndimage.zoom(a, f, a.dtype, order=2)) where the volumes of
test_gpu_zoom.py do not reach: end planes that scipy zeroes, outputs past the type's range, axes of one and two samples,
one-sample outputs, factors of 1 and above, lines long enough for z^(n-1) to underflow, and counts at the 256-lane block
edges of the three kernels.  Pure numpy: nothing here imports the package under test or scipy.  Where a case's name promises
a property the case carries it as data, and test_zoom_cases_host.py proves it against live scipy without a device.

The arithmetic restated here is scipy's own (ndimage/_interpolation.py zoom, ni_interpolation.c NI_ZoomShift):
    n_out = round(n_in * factor);   step = (n_in - 1) / (n_out - 1)  (1.0 when n_out == 1);   cc = k;  cc *= step
and with mode="constant" a coordinate cc > n_in - 1 gives cval = 0.  For some (n_in, n_out) the LAST cc overshoots n_in - 1
by one ulp, and the whole end plane of the output is zero.
"""
from collections import namedtuple

import numpy as np

POLE = -0.171572875253809902396622551580603843  # ni_splines.c, order 2
BLOCK = 256                                     # lanes per block of k_zoom_widen / k_zoom_prefilter / k_zoom_gather

# name, array, factor, and what the name promises (None / () where it promises nothing):
#   zero_axes   axes whose last output plane scipy zeroes (a tuple; () for a near miss that must not zero)
#   sides       which ends of the type's range the float64 result passes by more than 0.5: subset of ("hi", "lo")
#   long_axis   the axis whose line is long enough for POLE ** (n - 1) to be denormal or 0.0
#   line_counts {axis: number of prefilter lines along it} the name states
#   out_voxels  the output voxel count the name states
#   out_shape   the output shape scipy must give
ZoomCase = namedtuple("ZoomCase", "name array factor zero_axes sides long_axis line_counts out_voxels out_shape",
                      defaults=(None, None, None, None, None, None))

LIMITS = {np.dtype(np.int16): (-32768, 32767), np.dtype(np.uint8): (0, 255)}


def out_shape(shape, factor):
    """scipy's rule (and surface_process.resize_image_array's)"""
    return tuple(int(round(s * float(factor))) for s in shape)


def last_coordinate(n_in, n_out):
    """the float64 coordinate of the last output sample, computed as NI_ZoomShift does"""
    step = (n_in - 1) / (n_out - 1) if n_out > 1 else 1.0
    cc = float(n_out - 1)
    cc *= step
    return cc


def overshoots(n_in, n_out):
    return last_coordinate(n_in, n_out) > n_in - 1


def zeroed_axes(shape, factor):
    return tuple(ax for ax, (n, m) in enumerate(zip(shape, out_shape(shape, factor))) if m > 0 and overshoots(n, m))


def line_counts(shape):
    """{axis: lines along it}: the product of the other two extents"""
    d, h, w = shape
    return {0: h * w, 1: d * w, 2: d * h}


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31)


def hu_volume(shape, seed):
    """int16 noise in -1024..3071 without a single zero: a zero plane of the output cannot come from the data"""
    a = np.random.default_rng(seed).integers(-1024, 3072, shape).astype(np.int16)
    a[a == 0] = 1
    return a


def mask_volume(shape, seed, solid_end_axes=()):
    """uint8 mask of 0 / 255 / 254; the last three planes along each of `solid_end_axes` hold no zero"""
    rng = np.random.default_rng(seed + 1)
    m = rng.choice(np.array([0, 255, 254], np.uint8), size=shape, p=[0.45, 0.45, 0.1])
    for ax in solid_end_axes:
        sl = [slice(None)] * 3
        sl[ax] = slice(-3, None)
        end = m[tuple(sl)]
        end[end == 0] = 255
    return m


def bytes_volume(shape, seed):
    return np.random.default_rng(seed + 2).integers(0, 256, shape).astype(np.uint8)


def _pair(name, shape, factor, **props):
    """the int16 and the uint8 case of one shape"""
    s = _seed(name)
    axes = props.get("zero_axes") or ()
    return [ZoomCase(name + "-i16", hu_volume(shape, s), factor, **props),
            ZoomCase(name + "-u8", mask_volume(shape, s, axes) if "zero_axes" in props else bytes_volume(shape, s), factor, **props)]


# ---- end planes that scipy zeroes -------------------------------------------------------------------------------------------
# (id, shape, factor, axes with a zeroed end)
_ZERO_END = [
    ("zero-ax0-28", (28, 5, 6), 0.5, (0,)), ("zero-ax1-30", (5, 30, 6), 0.5, (1,)), ("zero-ax2-32", (5, 6, 32), 0.5, (2,)),
    ("zero-ax0-48", (48, 3, 4), 0.5, (0,)), ("zero-ax1-56", (3, 56, 4), 0.5, (1,)),
    ("zero-ax01-28x30", (28, 30, 7), 0.5, (0, 1)), ("zero-ax012-28x30x32", (28, 30, 32), 0.5, (0, 1, 2)),
    ("zero-ax0-320-medium", (320, 3, 4), 0.5, (0,)), ("zero-ax0-384-medium", (384, 3, 4), 0.5, (0,)),
    ("zero-ax0-600-medium", (600, 3, 4), 0.5, (0,)), ("zero-ax0-481-low", (481, 6, 7), 1 / 3.0, (0,)),
    ("zero-ax2-384-medium", (4, 6, 384), 0.5, (2,)), ("zero-ax1-320-medium", (3, 320, 4), 0.5, (1,)),
    ("zero-ax0-241-third", (241, 6, 7), 1 / 3.0, (0,)), ("zero-ax0-29-up-3over2", (29, 5, 6), 1.5, (0,)),
    # near misses: the last coordinate lands on n_in - 1 exactly
    ("nozero-ax0-34", (34, 5, 6), 0.5, ()), ("nozero-ax0-64", (64, 5, 6), 0.5, ()), ("nozero-ax0-240-third", (240, 6, 7), 1 / 3.0, ()),
    ("nozero-ax2-64", (5, 6, 64), 0.5, ()),
]
ZERO_END_CASES = [c for name, shape, f, axes in _ZERO_END for c in _pair(name, shape, f, zero_axes=axes)]


# ---- outputs past the type's range ---------------------------------------------------------------------------------------------
def _draw(values, dtype):
    return np.random.default_rng(1).choice(values, (9, 10, 11)).astype(dtype)


def _spike(shape, base, peak):
    a = np.full(shape, base, np.int16)
    a[tuple(s // 2 for s in shape)] = peak
    return a


def _checker(shape, cell):
    z, y, x = np.indices(shape)
    return (((z // cell + y // cell + x // cell) % 2) * 255).astype(np.uint8)


BOTH = ("hi", "lo")
CLAMP_CASES = [
    ZoomCase("clamp-i16-ends-draw-half", _draw([-32768, 32767], np.int16), 0.5, sides=BOTH),
    ZoomCase("clamp-i16-ends-draw-x2", _draw([-32768, 32767], np.int16), 2.0, sides=BOTH),
    ZoomCase("clamp-u8-ends-draw-half", _draw([0, 255], np.uint8), 0.5, sides=BOTH),
    ZoomCase("clamp-u8-ends-draw-x2", _draw([0, 255], np.uint8), 2.0, sides=BOTH),
    # one step of the full range: the spline rings below the floor around a spike and above the ceiling around a pit
    ZoomCase("clamp-i16-floor-one-spike-x2", _spike((5, 6, 7), -32768, 32767), 2.0, sides=("lo",)),
    ZoomCase("clamp-i16-ceiling-one-pit-x2", _spike((5, 6, 7), 32767, -32768), 2.0, sides=("hi",)),
    ZoomCase("clamp-i16-floor-one-spike-3over2", _spike((7, 8, 9), -32768, 32767), 1.5, sides=("lo",)),
    ZoomCase("clamp-i16-ceiling-one-pit-3over2", _spike((7, 8, 9), 32767, -32768), 1.5, sides=("hi",)),
    # cells of two voxels: steps, which overshoot both ways
    ZoomCase("clamp-u8-checker-cell2-x2", _checker((6, 7, 8), 2), 2.0, sides=BOTH),
    ZoomCase("clamp-u8-checker-cell2-3over2", _checker((6, 7, 8), 2), 1.5, sides=BOTH),
    # cells of one voxel: the Nyquist pattern, whose coefficients are eight times the data but whose spline never leaves
    # 0..255 -- nothing may clamp here
    ZoomCase("noclamp-u8-checker-cell1-x2", _checker((6, 7, 8), 1), 2.0, sides=()),
    ZoomCase("noclamp-u8-checker-cell1-half", _checker((7, 8, 9), 1), 0.5, sides=()),
]

# ---- axes of one and two samples, outputs of one sample, an empty output ----------------------------------------------------------
_SHORT = [
    ("short-in1-ax0-1x7x9-f0.6", (1, 7, 9), 0.6, (1, 4, 5)),
    ("short-in2-ax0-2x7x9-half", (2, 7, 9), 0.5, (1, 4, 4)),
    ("short-in2-all-2x2x2-half", (2, 2, 2), 0.5, (1, 1, 1)),
    ("short-in2-ax1-7x2x9-half", (7, 2, 9), 0.5, (4, 1, 4)),
    ("short-out1-ax0-3x6x9-third", (3, 6, 9), 1 / 3.0, (1, 2, 3)),
    ("short-identity-1x1x1", (1, 1, 1), 1.0, (1, 1, 1)),
    ("short-identity-5x6x7", (5, 6, 7), 1.0, (5, 6, 7)),
    ("short-empty-4x1x5-half", (4, 1, 5), 0.5, (2, 0, 2)),
    ("short-in2-ax0-2x3x4-x2", (2, 3, 4), 2.0, (4, 6, 8)),
    ("short-3x3x3-x3", (3, 3, 3), 3.0, (9, 9, 9)),
    ("short-in2-ax2-5x6x2-x2", (5, 6, 2), 2.0, (10, 12, 4)),
    ("short-in1-ax2-5x6x1-x2", (5, 6, 1), 2.0, (10, 12, 2)),
]
SHORT_CASES = [c for name, shape, f, osh in _SHORT for c in _pair(name, shape, f, out_shape=osh)]
IDENTITY_CASES = [c for c in SHORT_CASES if c.factor == 1.0]

# ---- long lines: POLE ** (n - 1) underflows --------------------------------------------------------------------------------------
_LONG = [("long-ax0-600-zero-end", (600, 2, 3), 0), ("long-ax1-600-zero-end", (2, 600, 3), 1), ("long-ax2-600-zero-end", (3, 2, 600), 2),
         ("long-ax0-450-pole-power-0", (450, 2, 3), 0), ("long-ax0-411-pole-power-denormal", (411, 2, 3), 0)]
LONG_CASES = [c for name, shape, ax in _LONG for c in _pair(name, shape, 0.5, long_axis=ax)]

# ---- counts at the edges of a 256-lane block ----------------------------------------------------------------------------------------
_BLOCK = [
    ("block-ax0-255-lines", (4, 15, 17), {0: 255}), ("block-ax0-256-lines", (4, 16, 16), {0: 256}), ("block-ax0-258-lines", (4, 6, 43), {0: 258}),
    ("block-ax1-255-lines", (15, 4, 17), {1: 255}), ("block-ax1-256-lines", (16, 4, 16), {1: 256}), ("block-ax1-258-lines", (6, 4, 43), {1: 258}),
    ("block-ax2-255-lines", (15, 17, 4), {2: 255}), ("block-ax2-256-lines", (16, 16, 4), {2: 256}), ("block-ax2-258-lines", (6, 43, 4), {2: 258}),
]
BLOCK_CASES = [c for name, shape, lc in _BLOCK for c in _pair(name, shape, 0.5, line_counts=lc)]
BLOCK_CASES += _pair("block-out-256-voxels", (8, 16, 16), 0.5, out_voxels=256)
BLOCK_CASES += _pair("block-out-257-voxels", (1, 1, 257), 1.0, out_voxels=257)

# ---- other factors -----------------------------------------------------------------------------------------------------------------
FACTOR_CASES = [c for f, tag in ((0.25, "quarter"), (0.75, "3over4"), (1.5, "3over2"), (2.0, "x2"))
                for c in _pair("factor-%s-11x14x9" % tag, (11, 14, 9), f, out_shape=out_shape((11, 14, 9), f))]

ALL_CASES = ZERO_END_CASES + CLAMP_CASES + SHORT_CASES + LONG_CASES + BLOCK_CASES + FACTOR_CASES
assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)


def ids(cases):
    return [c.name for c in cases]


def by_name(name):
    return next(c for c in ALL_CASES if c.name == name)
