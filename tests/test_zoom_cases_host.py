"""Every case of _zoom_cases.py stands where its name says, proven against live scipy without a device: the zeroed end planes
are zeroed by scipy (and only those), the clamp cases pass the type's range in float64 on the sides they name, the long lines
underflow the pole's power, the block-edge counts are the ones named, and the short axes give the shapes named."""
import functools
import math

import numpy as np
import pytest
from scipy import ndimage

import _zoom_cases as C


@functools.lru_cache(maxsize=None)
def _scipy(name):
    c = C.by_name(name)
    return ndimage.zoom(c.array, c.factor, c.array.dtype, order=2)


def _end_plane(a, axis, k=-1):
    return np.take(a, k, axis=axis)


def test_the_overshoot_rule_is_the_one_written_down():
    """the extents the cases are built on, by the float64 arithmetic alone: 28, 30, 32, 48, 56 (and 320, 384, 600) overshoot
    at 1/2 and 34, 64 do not; 241 and 481 at 1/3 and not 240; 29 at 3/2"""
    for n in (28, 30, 32, 48, 56, 320, 384, 600):
        assert C.overshoots(n, n // 2), n
    for n in (34, 64, 450, 411):
        assert not C.overshoots(n, int(round(n * 0.5))), n
    assert C.overshoots(241, 80) and C.overshoots(481, 160) and not C.overshoots(240, 80)
    assert C.overshoots(29, 44)
    # the product form a careless restatement would use lands on n_in - 1 exactly, every time
    for n_in, n_out in ((28, 14), (320, 160), (384, 192), (600, 300), (481, 160), (241, 80), (29, 44)):
        assert float(n_out - 1) * (n_in - 1) / (n_out - 1) == n_in - 1


@pytest.mark.parametrize("case", C.ZERO_END_CASES, ids=C.ids(C.ZERO_END_CASES))
def test_zeroed_end_cases(case):
    a, want = case.array, _scipy(case.name)
    assert C.zeroed_axes(a.shape, case.factor) == tuple(case.zero_axes)
    if a.dtype == np.int16:
        assert not (a == 0).any()
    else:
        assert set(np.unique(a)) <= {0, 254, 255}
    for ax in range(3):
        last, before = _end_plane(want, ax), _end_plane(want, ax, -2)
        if ax in case.zero_axes:
            assert not last.any(), "scipy does not zero the end of axis %d" % ax
            sl = [slice(None)] * 3
            sl[ax] = slice(-3, None)
            assert not (a[tuple(sl)] == 0).any(), "the zero plane could come from the data"
            # the plane before is real data (apart from the lines that end planes of OTHER axes zero)
            assert before.any()
        else:
            assert last.any(), "axis %d was not to be zeroed" % ax
    # exactly the promised planes, no more
    assert sum(not _end_plane(want, ax).any() for ax in range(3)) == len(case.zero_axes)


@pytest.mark.parametrize("case", C.CLAMP_CASES, ids=C.ids(C.CLAMP_CASES))
def test_clamp_cases(case):
    a, want = case.array, _scipy(case.name)
    lo, hi = C.LIMITS[a.dtype]
    f = ndimage.zoom(a, case.factor, np.float64, order=2)
    above, below = f > hi + 0.5, f < lo - 0.5
    assert bool(above.any()) == ("hi" in case.sides), int(above.sum())
    assert bool(below.any()) == ("lo" in case.sides), int(below.sum())
    assert (want[above] == hi).all() and (want[below] == lo).all()
    assert want.dtype == a.dtype and f.shape == want.shape


def test_clamp_draws_are_the_ones_counted():
    """the int16 draw at 1/2: 120 outputs, 18 above 32767.5 and 17 below -32768.5; at 2: thousands"""
    f = ndimage.zoom(C.by_name("clamp-i16-ends-draw-half").array, 0.5, np.float64, order=2)
    assert f.size == 120 and int((f > 32767.5).sum()) == 18 and int((f < -32768.5).sum()) == 17
    f = ndimage.zoom(C.by_name("clamp-i16-ends-draw-x2").array, 2.0, np.float64, order=2)
    assert f.size == 7920 and int((f > 32767.5).sum()) + int((f < -32768.5).sum()) > 1500


@pytest.mark.parametrize("case", C.LONG_CASES, ids=C.ids(C.LONG_CASES))
def test_long_line_cases(case):
    n = case.array.shape[case.long_axis]
    assert n == max(case.array.shape)
    p = abs(math.pow(C.POLE, n - 1))
    assert p < 2.2250738585072014e-308  # below the smallest normal double: denormal or 0.0
    if "denormal" in case.name:
        assert p > 0.0
    if "power-0" in case.name:
        assert p == 0.0
    zero_end = "zero-end" in case.name
    assert (case.long_axis in C.zeroed_axes(case.array.shape, case.factor)) == zero_end
    assert (not _end_plane(_scipy(case.name), case.long_axis).any()) == zero_end


@pytest.mark.parametrize("case", C.BLOCK_CASES, ids=C.ids(C.BLOCK_CASES))
def test_block_edge_cases(case):
    shape = case.array.shape
    if case.line_counts is not None:
        for ax, n in case.line_counts.items():
            assert C.line_counts(shape)[ax] == n and ("ax%d-%d-lines" % (ax, n)) in case.name
            assert n in (C.BLOCK - 1, C.BLOCK) or C.BLOCK < n <= C.BLOCK + 2
            assert shape[ax] > 1  # (a line of one sample is not filtered: no launch)
    if case.out_voxels is not None:
        assert int(np.prod(_scipy(case.name).shape)) == case.out_voxels and ("out-%d-voxels" % case.out_voxels) in case.name


def test_block_edges_cover_each_axis_on_both_sides():
    for ax in range(3):
        counts = sorted(c.line_counts[ax] for c in C.BLOCK_CASES if c.line_counts and ax in c.line_counts and c.array.dtype == np.int16)
        assert counts[:2] == [255, 256] and counts[2] > 256
    outs = {c.out_voxels for c in C.BLOCK_CASES if c.out_voxels}
    assert 256 in outs and 257 in outs


@pytest.mark.parametrize("case", C.SHORT_CASES + C.FACTOR_CASES, ids=C.ids(C.SHORT_CASES + C.FACTOR_CASES))
def test_short_axis_and_factor_cases(case):
    want = _scipy(case.name)
    assert want.shape == tuple(case.out_shape) == C.out_shape(case.array.shape, case.factor)
    assert want.dtype == case.array.dtype


def test_short_cases_reach_each_branch():
    shapes = [(c.array.shape, tuple(c.out_shape)) for c in C.SHORT_CASES]
    for ax in range(3):
        assert any(i[ax] == 2 and min(o) > 0 for i, o in shapes), "no two-sample line along axis %d" % ax
    assert any(i[0] == 1 and o[0] == 1 for i, o in shapes) and any(i[2] == 1 and o[2] == 2 for i, o in shapes)
    assert any(i[0] == 3 and o[0] == 1 for i, o in shapes)  # a one-sample output of a longer line: scipy's step is 1.0
    assert any(0 in o for i, o in shapes)
    # the two-sample cases are not symmetric along that line, so reading sample 0 for sample 1 changes the result
    for c in C.SHORT_CASES:
        for ax in range(3):
            if c.array.shape[ax] == 2:
                assert not np.array_equal(np.take(c.array, 0, axis=ax), np.take(c.array, 1, axis=ax)), c.name


@pytest.mark.parametrize("case", C.IDENTITY_CASES, ids=C.ids(C.IDENTITY_CASES))
def test_factor_one_is_the_identity(case):
    assert np.array_equal(_scipy(case.name), case.array)


def test_every_volume_is_small():
    for c in C.ALL_CASES:
        assert c.array.size <= 50000 and c.array.dtype in (np.int16, np.uint8), c.name
        assert int(np.prod(C.out_shape(c.array.shape, c.factor))) <= 50000, c.name
