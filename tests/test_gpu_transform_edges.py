"""GPU parity of apply_view_matrix_transform (csrc/k_transform.hip) with the C oracle, away from the int16 / AXIAL / identity
corner that tests/test_gpu_transform.py covers: every dtype under a real matrix, every placement, Lanczos on float64, a cval above
part of the data, the NumCast bounds, the edges of the inside test, short axes, homogeneous rows, strided views, the second trip
of the grid-stride loop, and the argument surface.  The cases come from tests/_transform_cases.py; tests/test_oracle_transform.py
holds the oracle, on the same cases, against an independent restatement on the CPU."""
import numpy as np
import pytest

import _transform_cases as tc

pytestmark = pytest.mark.gpu

MODES_EXACT = [0, 1, 2]
_IDS = [p[0] for p in tc.PLACEMENTS]


def _rs():
    from invesalius3_amd import invesalius_rs
    return invesalius_rs.apply_view_matrix_transform


def _pair(oracle, vol, spacing, M, n, orientation, minterpol, cval, oshape):
    g = tc.run(_rs(), vol, spacing, M, n, orientation, minterpol, cval, oshape, fill=0)
    r = tc.run(oracle.apply_view_matrix_transform, vol, spacing, M, n, orientation, minterpol, cval, oshape, fill=0)
    return g, r


def _assert_same(g, r):
    assert np.array_equal(g, r), np.argwhere(g != r)[:4]
    if g.dtype == np.float64:
        assert np.array_equal(g.view(np.uint64), r.view(np.uint64))


def _assert_one_lsb(g, r):
    dmax, ndiff, allowed = tc.one_lsb(g, r)
    print("Lanczos integer: max |g - r| = %d on %d of %d voxels (allowed %d)" % (dmax, ndiff, g.size, allowed))
    assert dmax <= 1 and ndiff <= allowed


def _assert_lanczos_f64(g, r, S):
    """|g - r| <= 32 eps S.  Both sides run the same IEEE products and sums and differ only in sin(): two calls per weight, three
    weights per term, the device's documented at <= 2 ulp and glibc's below 1 -- under 16 ulp of each term, doubled for slack in
    the accumulation.  Returns the measured max |g - r| / (eps S)."""
    err = np.abs(g - r)
    assert (err[S == 0] == 0).all()  # outside voxels: cval on both sides
    ratio = float((err[S > 0] / (tc.EPS * S[S > 0])).max())
    print("Lanczos float64: max |g - r| / (eps S) = %.3f over %d inside voxels" % (ratio, int((S > 0).sum())))
    assert (err <= 32.0 * tc.EPS * S).all(), ratio
    return ratio


# ---- 1. parity matrix -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orientation,n,oshape", tc.PLACEMENTS, ids=_IDS)
@pytest.mark.parametrize("minterpol", MODES_EXACT)
@pytest.mark.parametrize("dtype", tc.DTYPES, ids=["u8", "i16", "f64"])
def test_parity_matrix(ivxlib, oracle, dtype, minterpol, orientation, n, oshape):
    vol = tc.volume(dtype)
    M = tc.matrix()
    g, r = _pair(oracle, vol, tc.SPACING, M, n, orientation, minterpol, vol.min().item(), oshape)
    _assert_same(g, r)
    assert tc.source_coords(vol.shape, tc.SPACING, M, n, orientation, oshape)[3].mean() > 0.5


# ---- 2. Lanczos, integer dtypes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("orientation,n,oshape", tc.PLACEMENTS, ids=_IDS)
@pytest.mark.parametrize("dtype", [np.uint8, np.int16], ids=["u8", "i16"])
def test_lanczos_integer_within_one_lsb(ivxlib, oracle, dtype, orientation, n, oshape):
    vol = tc.volume(dtype)
    g, r = _pair(oracle, vol, tc.SPACING, tc.matrix(), n, orientation, 3, vol.min().item(), oshape)
    _assert_one_lsb(g, r)


# ---- 3. Lanczos, float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orientation,n,oshape", tc.PLACEMENTS, ids=_IDS)
def test_lanczos_float64_within_sin_error(ivxlib, oracle, orientation, n, oshape):
    """No truncating cast hides a wrong weight here.  cval = -1e300, so the clamp plays no part.
    Measured on an MI355X: max |g - r| / (eps S) = 0.782 (AXIAL), 0.823 (CORONAL), 0.782 (SAGITAL), 1.282 (OTHER); the bound is 32."""
    vol = tc.volume(np.float64)
    M = tc.matrix()
    g, r = _pair(oracle, vol, tc.SPACING, M, n, orientation, 3, -1e300, oshape)
    S, inside = tc.lanczos_abs_sum(vol, tc.SPACING, M, n, orientation, oshape)
    assert inside.mean() > 0.5 and (g[~inside] == -1e300).all() and (g[inside] != -1e300).all()
    _assert_lanczos_f64(g, r, S)


# ---- 4. cval above part of the data -----------------------------------------------------------------------------------
@pytest.mark.parametrize("minterpol", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype,cval", [(np.int16, 0), (np.float64, 31.25)], ids=["i16", "f64"])
def test_cval_above_part_of_the_data(ivxlib, oracle, dtype, cval, minterpol):
    """the clamp v < cval -> cval belongs to tricubic and Lanczos alone (transforms.rs:35-50)"""
    vol = tc.volume(dtype)
    orientation, n, oshape = tc.OTHER
    M = tc.matrix()
    g, r = _pair(oracle, vol, tc.SPACING, M, n, orientation, minterpol, cval, oshape)
    if minterpol < 3:
        _assert_same(g, r)
    elif dtype is np.int16:
        _assert_one_lsb(g, r)
    else:
        _assert_lanczos_f64(g, r, tc.lanczos_abs_sum(vol, tc.SPACING, M, n, orientation, oshape)[0])
    assert (g < cval).any() == (minterpol in (0, 1))
    assert (g > cval).any()


# ---- 5. cast bounds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,c,p3,exact,result", tc.CAST_PROFILES)
def test_cast_bounds(ivxlib, oracle, dtype, c, p3, exact, result):
    """NumCast accepts the open interval (MIN - 1, MAX + 1) and truncates toward zero: MIN - 0.375 and MAX + 0.375 are values,
    one step further is the reference's panic"""
    vol = tc.cast_volume(dtype, c, p3)
    cval = int(np.iinfo(dtype).min)
    args = (vol, (1.0, 1.0, 1.0), tc.cast_matrix(), tc.CAST_N, "AXIAL", 2, cval)
    if result is None:
        g, r = np.full(tc.CAST_OSHAPE, 7, dtype), np.full(tc.CAST_OSHAPE, 7, dtype)
        with pytest.raises(ValueError):
            oracle.apply_view_matrix_transform(*args, r)
        with pytest.raises(ValueError):
            _rs()(*args, g)
        assert np.array_equal(g, r) and (g[0, :5, 3] == cval).all()  # the failing voxels hold cval
    else:
        g, r = _pair(oracle, *args, tc.CAST_OSHAPE)
        _assert_same(g, r)
        assert (g[0, :5, 3] == result).all()


def test_trilinear_truncates_toward_zero(ivxlib, oracle):
    vol = tc.cast_volume(np.int16, -4, -4)
    vol[:, :, 4] = -3
    g, r = _pair(oracle, vol, (1.0, 1.0, 1.0), tc.cast_matrix(), tc.CAST_N, "AXIAL", 1, -100, tc.CAST_OSHAPE)
    _assert_same(g, r)
    assert (g[0, :5, 3] == -3).all()  # -3.5 -> -3


# ---- 6. the inside test's edges ---------------------------------------------------------------------------------------
EDGE_SHAPE = (5, 6, 7)
EDGE_CVAL = -1000


def _edge_volume(shape=EDGE_SHAPE):
    return np.random.default_rng(5).integers(-900, 1000, shape).astype(np.int16)


def _shifted(vol, axis, t, cval):
    """nearest, spacing 1: out[c] = vol[c + t e_axis] where 0 <= c + t e_axis < d - 1 on every axis, cval elsewhere"""
    out = np.full(vol.shape, cval, vol.dtype)
    idx = np.indices(vol.shape)
    src = [idx[a] + (t if a == axis else 0) for a in range(3)]
    ok = np.ones(vol.shape, bool)
    for a in range(3):
        ok &= (src[a] >= 0) & (src[a] < vol.shape[a] - 1)
    out[ok] = vol[src[0][ok], src[1][ok], src[2][ok]]
    return out


_SHIFTS = [(a, t) for a in range(3) for t in (-1, 0, 1, EDGE_SHAPE[a] - 2)]


@pytest.mark.parametrize("axis,t", _SHIFTS)
def test_translation_edges_unit_spacing(ivxlib, oracle, axis, t):
    vol = _edge_volume()
    sp = (1.0, 1.0, 1.0)
    M = tc.translation(axis, t, sp)
    for minterpol in MODES_EXACT:
        g, r = _pair(oracle, vol, sp, M, 0, "OTHER", minterpol, EDGE_CVAL, EDGE_SHAPE)
        _assert_same(g, r)
        if minterpol == 0:
            assert np.array_equal(g, _shifted(vol, axis, t, EDGE_CVAL))
            if t >= 0:  # the source's last slice, row and column are never inside (n < d - 1)
                assert (g[-1] == EDGE_CVAL).all() and (g[:, -1] == EDGE_CVAL).all() and (g[:, :, -1] == EDGE_CVAL).all()
            assert (g != EDGE_CVAL).any()


@pytest.mark.parametrize("axis,t", _SHIFTS)
def test_translation_edges_real_spacing(ivxlib, oracle, axis, t):
    """(x s) / s need not return x: which side of 0 and of d - 1 a voxel lands on is the oracle's to say, bit for bit"""
    vol = _edge_volume()
    sp = (0.4785156, 0.4785156, 1.25)
    M = tc.translation(axis, t, sp)
    for minterpol in MODES_EXACT:
        g, r = _pair(oracle, vol, sp, M, 0, "OTHER", minterpol, EDGE_CVAL, EDGE_SHAPE)
        _assert_same(g, r)


def _quarter_shift():
    M = np.eye(4)
    M[:3, 3] = 0.25
    return M


@pytest.mark.parametrize("shape", [(1, 6, 7), (5, 1, 7), (5, 6, 1)])
def test_axis_of_length_1_is_all_cval(ivxlib, oracle, shape):
    vol = _edge_volume(shape)
    for M in (np.eye(4), _quarter_shift()):
        for minterpol in (0, 1, 2, 3):
            g, r = _pair(oracle, vol, (1.0, 1.0, 1.0), M, 0, "OTHER", minterpol, EDGE_CVAL, shape)
            assert (g == EDGE_CVAL).all() and (r == EDGE_CVAL).all()


@pytest.mark.parametrize("shape", [(2, 6, 7), (5, 2, 7), (5, 6, 2)])
def test_axis_of_length_2_exact_modes(ivxlib, oracle, shape):
    vol = _edge_volume(shape)
    for M in (np.eye(4), _quarter_shift()):
        for minterpol in MODES_EXACT:
            g, r = _pair(oracle, vol, (1.0, 1.0, 1.0), M, 0, "OTHER", minterpol, EDGE_CVAL, shape)
            _assert_same(g, r)
            if minterpol < 2:  # (tricubic may undershoot below cval and be clamped to it)
                assert (g != EDGE_CVAL).sum() == (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)


# ---- 7. Lanczos on short axes -----------------------------------------------------------------------------------------
def test_lanczos_smallest_legal_volume(ivxlib, oracle):
    """(3, 4, 5): the tap floor(x) - 3 = -3 wraps to 0 on the axis of length 3 -- the last in-bounds case"""
    vol = _edge_volume((3, 4, 5))
    g, r = _pair(oracle, vol, (1.0, 1.0, 1.0), _quarter_shift(), 0, "OTHER", 3, EDGE_CVAL, (3, 4, 5))
    _assert_one_lsb(g, r)
    assert (g != EDGE_CVAL).any()


@pytest.mark.parametrize("shape", [(2, 6, 7), (5, 2, 7), (5, 6, 2)])
def test_lanczos_axis_of_length_2_is_the_reference_panic(ivxlib, oracle, shape):
    """On an axis of length 2 the tap -3 wraps once to -1, which the reference indexes as usize: a panic.  Here: ValueError, the
    voxel set to cval, nothing read.  A matrix that maps every voxel outside never reaches the taps: all cval, no error."""
    vol = _edge_volume(shape)
    sp = (1.0, 1.0, 1.0)
    for M in (np.eye(4), _quarter_shift()):
        g, r = np.full(shape, 77, np.int16), np.full(shape, 77, np.int16)
        with pytest.raises(ValueError):
            oracle.apply_view_matrix_transform(vol, sp, M, 0, "OTHER", 3, EDGE_CVAL, r)
        with pytest.raises(ValueError):
            _rs()(vol, sp, M, 0, "OTHER", 3, EDGE_CVAL, g)
        assert (g == EDGE_CVAL).all() and (r == EDGE_CVAL).all()
    g, r = _pair(oracle, vol, sp, tc.translation(1, 100, sp), 0, "OTHER", 3, EDGE_CVAL, shape)
    assert (g == EDGE_CVAL).all() and (r == EDGE_CVAL).all()


# ---- 8. homogeneous row -----------------------------------------------------------------------------------------------
def _homogeneous(kind):
    M = tc.matrix()
    if kind == "w":
        M[3, 3] = 1.25
    elif kind == "row":
        M[3, :3] = (1e-3, -2e-3, 5e-4)
    else:
        M[3, :] = 0.0
    return M


@pytest.mark.parametrize("kind", ["w", "row", "zero"])
def test_homogeneous_row(ivxlib, oracle, kind):
    vol = tc.volume(np.int16)
    cval = int(vol.min())
    orientation, n, oshape = tc.OTHER
    for minterpol in MODES_EXACT:
        g, r = _pair(oracle, vol, tc.SPACING, _homogeneous(kind), n, orientation, minterpol, cval, oshape)
        _assert_same(g, r)
        if kind == "zero":
            assert (g == cval).all()  # every coordinate is inf or NaN
        else:
            plain = tc.run(oracle.apply_view_matrix_transform, vol, tc.SPACING, tc.matrix(), n, orientation, minterpol, cval, oshape)
            assert (g != cval).mean() > 0.3 and (g != plain).any()


# ---- 9. views ---------------------------------------------------------------------------------------------------------
SENTINEL = 12345


def _volume_views():
    vol = tc.volume(np.int16)
    big = np.full((10, 12, 14), SENTINEL, np.int16)
    big[1:, 1:, 1:] = vol
    wide = np.full((9, 11, 26), SENTINEL, np.int16)
    wide[:, :, ::2] = vol
    return {"interior": (big, big[1:, 1:, 1:]), "every_other_x": (wide, wide[:, :, ::2]),
            "fortran": (None, np.asfortranarray(vol)), "reversed_z": (vol, vol[::-1])}


@pytest.mark.parametrize("name", ["interior", "every_other_x", "fortran", "reversed_z"])
def test_volume_views(ivxlib, oracle, name):
    parent, view = _volume_views()[name]
    assert not view.flags["C_CONTIGUOUS"]
    before = None if parent is None else parent.copy()
    dense = np.ascontiguousarray(view)
    orientation, n, oshape = tc.OTHER
    for minterpol in (0, 1):
        g = tc.run(_rs(), view, tc.SPACING, tc.matrix(), n, orientation, minterpol, -4000, oshape)
        d = tc.run(_rs(), dense, tc.SPACING, tc.matrix(), n, orientation, minterpol, -4000, oshape)
        r = tc.run(oracle.apply_view_matrix_transform, dense, tc.SPACING, tc.matrix(), n, orientation, minterpol, -4000, oshape)
        assert np.array_equal(g, d) and np.array_equal(g, r)
        assert (g != -4000).mean() > 0.5
    assert before is None or np.array_equal(parent, before)


@pytest.mark.parametrize("name", ["interior", "every_other_x", "reversed_z"])
def test_output_views(ivxlib, oracle, name):
    vol = tc.volume(np.int16)
    orientation, n, oshape = tc.OTHER
    want = tc.run(_rs(), vol, tc.SPACING, tc.matrix(), n, orientation, 1, -4000, oshape)
    assert (want != SENTINEL).all()
    if name == "interior":
        big = np.full((11, 13, 15), SENTINEL, np.int16)
        out = big[1:-1, 1:-1, 1:-1]
    elif name == "every_other_x":
        big = np.full((9, 11, 26), SENTINEL, np.int16)
        out = big[:, :, ::2]
    else:
        big = np.full((10, 11, 13), SENTINEL, np.int16)
        out = big[:0:-1]
    _rs()(vol, tc.SPACING, tc.matrix(), n, orientation, 1, -4000, out)
    assert np.array_equal(out, want)
    assert (big == SENTINEL).sum() == big.size - want.size  # every sentinel outside the view survives


# ---- 10. second trip of the grid-stride loop --------------------------------------------------------------------------
@pytest.mark.parametrize("minterpol", [0, 1])
def test_grid_stride_second_trip(ivxlib, oracle, minterpol):
    """65 * 512 * 512 = 17 039 360 output voxels, past the 65536 blocks of 256 lanes the launch is capped at: the voxels from
    16 777 216 on -- all of the last slice -- are written on the loop's second trip.  Every voxel is inside."""
    vol = tc.volume(np.uint8)
    oshape = (65, 512, 512)
    assert oshape[0] * oshape[1] * oshape[2] > 65536 * 256 and 64 * 512 * 512 >= 65536 * 256
    sp = (1.0, 1.0, 1.0)
    M = np.diag([8.0 / 65.0, 10.0 / 512.0, 12.0 / 512.0, 1.0])
    assert all(0.0 <= (o - 1) * M[a, a] < d - 1.0 for a, (o, d) in enumerate(zip(oshape, vol.shape)))  # the far corner is inside
    g = tc.run(_rs(), vol, sp, M, 0, "OTHER", minterpol, 0, oshape, fill=1)
    r = tc.run(oracle.apply_view_matrix_transform, vol, sp, M, 0, "OTHER", minterpol, 0, oshape, fill=2)
    assert len(np.unique(r[64])) >= 50
    assert np.array_equal(g[64], r[64]), "the second trip of the grid-stride loop"
    assert np.array_equal(g[:64], r[:64])


# ---- 11. argument surface ---------------------------------------------------------------------------------------------
def test_argument_surface(ivxlib, oracle):
    vol = tc.volume(np.int16)
    cval = int(vol.min())
    M = tc.matrix()
    with pytest.raises(OverflowError):  # `n: usize` (transforms_py.rs:100)
        _rs()(vol, tc.SPACING, M, -1, "AXIAL", 0, cval, np.zeros((3, 11, 13), np.int16))
    g = tc.run(_rs(), vol, tc.SPACING, M, 1000, "AXIAL", 1, cval, (3, 11, 13), fill=5)
    assert (g == cval).all()  # n beyond the volume
    orientation, n, oshape = tc.PLACEMENTS[0]
    lanczos = tc.run(_rs(), vol, tc.SPACING, M, n, orientation, 3, cval, oshape)
    for minterpol in (4, -1):  # `_ =>` of transforms.rs:43
        g, r = _pair(oracle, vol, tc.SPACING, M, n, orientation, minterpol, cval, oshape)
        assert np.array_equal(g, lanczos)
        _assert_one_lsb(g, r)
    other = tc.run(_rs(), vol, tc.SPACING, M, 5, "OTHER", 1, cval, tc.SHAPE)
    for name in ("axial", "", "VOLUME"):  # an unknown orientation string: no offset, n ignored
        g, r = _pair(oracle, vol, tc.SPACING, M, 5, name, 1, cval, tc.SHAPE)
        _assert_same(g, r)
        assert np.array_equal(g, other)
