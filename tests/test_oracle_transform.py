"""A SECOND, independent restatement of invesalius_rs/src/transforms.rs + interpolation.rs (apply_view_matrix_transform: the
resampler behind a reoriented view, invesalius/data/slice_.py:862-874) in plain Python floats -- IEEE doubles, the Rust
source's operation order -- against which oracle/'s C restatement must agree bit for bit.  Upstream has no test for it;
oracle/ was cross-checked against scipy for nearest / trilinear only, so the tricubic and Lanczos-4 branches rested on one
transcription.

  coord_transform                 transforms.rs:9-55     (z, y, x, 1) * spacing -> m -> / w -> / spacing; inside test; cval clamp
  get_value                       interpolation.rs:6-35  one wrap-around step per axis
  trilinear / tricubic / lanczos  interpolation.rs:63-188"""
import math

import numpy as np
import pytest

import _transform_cases as tc


def _get(v, x, y, z):
    dz, dy, dx = v.shape
    x = x + dx if x < 0 else (x - dx if x >= dx else x)
    y = y + dy if y < 0 else (y - dy if y >= dy else y)
    z = z + dz if z < 0 else (z - dz if z >= dz else z)
    if x < 0 or y < 0 or z < 0:
        raise ValueError("index %r as usize" % ((z, y, x),))  # interpolation.rs:34: the reference panics, numpy would wrap again
    return float(v[z, y, x])


def _cubic(p, x):
    return p[1] + 0.5 * x * (p[2] - p[0] + x * (2.0 * p[0] - 5.0 * p[1] + 4.0 * p[2] - p[3] + x * (3.0 * (p[1] - p[2]) + p[3] - p[0])))


def _bicubic(p, x, y):
    return _cubic([_cubic(p[0], y), _cubic(p[1], y), _cubic(p[2], y), _cubic(p[3], y)], x)


def _lanczos_kernel(x, a):
    if x == 0.0:
        return 1.0
    if -float(a) <= x < float(a):
        af = float(a)
        return (af * math.sin(math.pi * x) * math.sin(math.pi * (x / af))) / (math.pi * math.pi * x * x)
    return 0.0


def _trilinear(v, x, y, z):
    x0, y0, z0 = math.floor(x), math.floor(y), math.floor(z)
    x1, y1, z1 = x0 + 1, y0 + 1, z0 + 1
    xd, yd, zd = x - x0, y - y0, z - z0
    c00 = _get(v, x0, y0, z0) * (1.0 - xd) + _get(v, x1, y0, z0) * xd
    c10 = _get(v, x0, y1, z0) * (1.0 - xd) + _get(v, x1, y1, z0) * xd
    c01 = _get(v, x0, y0, z1) * (1.0 - xd) + _get(v, x1, y0, z1) * xd
    c11 = _get(v, x0, y1, z1) * (1.0 - xd) + _get(v, x1, y1, z1) * xd
    c0 = c00 * (1.0 - yd) + c10 * yd
    c1 = c01 * (1.0 - yd) + c11 * yd
    return c0 * (1.0 - zd) + c1 * zd


def _tricubic(v, x, y, z):
    xi, yi, zi = math.floor(x), math.floor(y), math.floor(z)
    p = [[[_get(v, xi + i - 1, yi + j - 1, zi + k - 1) for k in range(4)] for j in range(4)] for i in range(4)]
    arr = [_bicubic(p[i], y - yi, z - zi) for i in range(4)]
    return _cubic(arr, x - xi)


def _lanczos(v, x, y, z):
    a = 4
    xd, yd, zd = math.floor(x), math.floor(y), math.floor(z)
    xs, ys, zs = range(xd - a + 1, xd + a), range(yd - a + 1, yd + a), range(zd - a + 1, zd + a)
    temp_y = []
    for kk in zs:
        ly = 0.0
        for jj in ys:
            lx = 0.0
            for ii in xs:
                lx += _get(v, ii, jj, kk) * _lanczos_kernel(x - ii, a)
            ly += lx * _lanczos_kernel(y - jj, a)
        temp_y.append(ly)
    lz = 0.0
    for m, kk in enumerate(zs):
        lz += temp_y[m] * _lanczos_kernel(z - kk, a)
    return lz


def _div(a, b):
    """IEEE division: x / 0 is inf or NaN as in Rust, where Python floats raise"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


_CAST_BOUNDS = {np.dtype(np.int16): (-32769.0, 32768.0), np.dtype(np.uint8): (-1.0, 256.0)}


def _numcast(f, dtype):
    """NumCast::from(f64) -> T (num-traits: inside the open interval (MIN - 1, MAX + 1), then truncation toward zero; NaN fails);
    f64 -> f64 is the identity"""
    if dtype.kind == "f":
        return f
    lo, hi = _CAST_BOUNDS[dtype]
    if not lo < f < hi:
        raise ValueError("NumCast")
    return int(f)


def transform_py(volume, spacing, m, n, orientation, minterpol, cval, out_shape, errors=None):
    """int16, uint8 and float64.  Where the reference would panic -- a NumCast failure, or the index -1 that a Lanczos tap reaches
    on an axis of length 2 -- ValueError; with a list as `errors` the voxel is recorded there, set to cval, and the loop goes on
    (what the C oracle and the kernel leave behind before they report)."""
    sx, sy, sz = (float(s) for s in spacing)
    dz, dy, dx = (float(s) for s in volume.shape)
    out = np.zeros(out_shape, volume.dtype)
    M = [[float(m[r][c]) for c in range(4)] for r in range(4)]
    for cz in range(out_shape[0]):
        for cy in range(out_shape[1]):
            for cx in range(out_shape[2]):
                z, y, x = cz, cy, cx
                if orientation == "AXIAL":
                    z = n + cz
                elif orientation == "CORONAL":
                    y = n + cy
                elif orientation == "SAGITAL":
                    x = n + cx
                c = (z * sz, y * sy, x * sx, 1.0)
                nc = [M[r][0] * c[0] + M[r][1] * c[1] + M[r][2] * c[2] + M[r][3] * c[3] for r in range(4)]
                nz, ny, nx = _div(_div(nc[0], nc[3]), sz), _div(_div(nc[1], nc[3]), sy), _div(_div(nc[2], nc[3]), sx)
                if 0.0 <= nz < dz - 1.0 and 0.0 <= ny < dy - 1.0 and 0.0 <= nx < dx - 1.0:
                    try:
                        if minterpol == 0:
                            val = volume[int(nz), int(ny), int(nx)]
                        elif minterpol == 1:
                            val = _numcast(_trilinear(volume, nx, ny, nz), volume.dtype)
                        else:
                            val = _numcast(_tricubic(volume, nx, ny, nz) if minterpol == 2 else _lanczos(volume, nx, ny, nz), volume.dtype)
                            val = cval if val < cval else val
                    except ValueError:
                        if errors is None:
                            raise
                        errors.append((cz, cy, cx))
                        val = cval
                    out[cz, cy, cx] = val
                else:
                    out[cz, cy, cx] = cval
    return out


def _rotation(rng):
    a, b, c = rng.uniform(-0.6, 0.6, 3)
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    rx = np.array([[1, 0, 0], [0, math.cos(c), -math.sin(c)], [0, math.sin(c), math.cos(c)]])
    return rz @ ry @ rx


@pytest.mark.parametrize("minterpol", [0, 1, 2, 3])
def test_view_matrix_transform_second_restatement(oracle, minterpol):
    rng = np.random.default_rng(40 + minterpol)
    inside = 0
    for trial in range(6):
        shape = tuple(int(v) for v in rng.integers(6, 11, 3))
        vol = rng.integers(-900, 1000, shape).astype(np.int16)
        spacing = tuple(float(v) for v in rng.uniform(0.5, 2.0, 3))
        m = np.eye(4)
        m[:3, :3] = _rotation(rng)
        centre = np.array([shape[0] * spacing[2], shape[1] * spacing[1], shape[2] * spacing[0]]) / 2.0
        m[:3, 3] = centre - m[:3, :3] @ centre + rng.uniform(-1.0, 1.0, 3)  # rotate about the centre, nudge
        if trial == 5:
            m[3, 3] = 1.25  # a homogeneous coordinate that is not 1
        orientation = ["AXIAL", "CORONAL", "SAGITAL", "OTHER"][trial % 4]
        n = int(rng.integers(0, 3))
        oshape = [shape[0], shape[1], shape[2]]
        oshape[trial % 3] = 2 if orientation != "OTHER" else oshape[trial % 3]  # the reference resamples thin slabs
        cval = int(vol.min())
        got = np.zeros(oshape, np.int16)
        oracle.apply_view_matrix_transform(vol, spacing, m, n, orientation, minterpol, cval, got)
        want = transform_py(vol, spacing, m, n, orientation, minterpol, cval, tuple(oshape))
        assert np.array_equal(got, want), (trial, orientation, np.argwhere(got != want)[:3])
        inside += int((want != cval).sum())
    assert inside > 200  # the slabs do hit the volume


# ---- the shared cases of tests/_transform_cases.py: the GPU tests compare the kernel with the C oracle on them, so the C oracle is
# held here, on the same inputs, against the restatement above -----------------------------------------------------------------
def _both(oracle, vol, spacing, m, n, orientation, minterpol, cval, oshape):
    """(oracle's output, restatement's output, oracle raised, restatement's failing voxels)"""
    got = np.full(oshape, 77, vol.dtype)
    raised = False
    try:
        oracle.apply_view_matrix_transform(vol, spacing, m, n, orientation, minterpol, cval, got)
    except ValueError:
        raised = True
    errors = []
    want = transform_py(vol, spacing, m, n, orientation, minterpol, cval, tuple(oshape), errors)
    return got, want, raised, errors


@pytest.mark.parametrize("minterpol", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_restatement_uint8_float64(oracle, dtype, minterpol):
    """uint8 goes through NumCast (truncation toward zero), float64 through no cast at all: Lanczos included, the oracle and the
    restatement call the same libm sin in the same order, so float64 is compared by bits"""
    vol = tc.volume(dtype)
    cval = vol.min().item()
    inside = 0
    for orientation, n, oshape in tc.PLACEMENTS[1:]:
        got, want, raised, errors = _both(oracle, vol, tc.SPACING, tc.matrix(), n, orientation, minterpol, cval, oshape)
        assert not raised and not errors
        if dtype is np.float64:
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        assert np.array_equal(got, want)
        inside += int(tc.source_coords(vol.shape, tc.SPACING, tc.matrix(), n, orientation, oshape)[3].sum())
        if dtype is np.float64 and minterpol in (1, 2):
            assert (got != np.trunc(got)).any()  # nothing truncated it
    assert inside > 1000


def test_numcast_failure_leaves_cval_and_reports(oracle):
    """the checkerboard of the GPU test: uint8 tricubic overshoot; the failing voxels hold cval, the others their value"""
    v = np.zeros((8, 8, 8), np.uint8)
    v[:, :, 3:5] = 255
    got, want, raised, errors = _both(oracle, v, (1.0, 1.0, 1.0), tc.cast_matrix(), 2, "AXIAL", 2, 9, (2, 8, 8))
    assert raised and errors and np.array_equal(got, want)
    assert all(got[e] == 9 for e in errors)


@pytest.mark.parametrize("dtype,cval", [(np.int16, 0), (np.float64, 31.25)])
@pytest.mark.parametrize("minterpol", [0, 1, 2, 3])
def test_cval_above_part_of_the_data(oracle, dtype, cval, minterpol):
    """v < cval -> cval for tricubic and Lanczos only (transforms.rs:35-50): nearest and trilinear keep what lies below"""
    vol = tc.volume(dtype)
    assert (vol < cval).mean() > 0.05
    orientation, n, oshape = tc.OTHER
    got, want, raised, errors = _both(oracle, vol, tc.SPACING, tc.matrix(), n, orientation, minterpol, cval, oshape)
    assert not raised and not errors and np.array_equal(got, want)
    assert (got < cval).any() == (minterpol in (0, 1))


@pytest.mark.parametrize("dtype,c,p3,exact,result", tc.CAST_PROFILES)
def test_cast_bound_profiles(oracle, dtype, c, p3, exact, result):
    vol = tc.cast_volume(dtype, c, p3)
    p = [float(c), float(c), float(c), float(p3)]
    assert _cubic(p, 0.5) == exact == (-p[0] + 9 * p[1] + 9 * p[2] - p[3]) / 16
    cval = int(np.iinfo(dtype).min)
    got, want, raised, errors = _both(oracle, vol, (1.0, 1.0, 1.0), tc.cast_matrix(), tc.CAST_N, "AXIAL", 2, cval, tc.CAST_OSHAPE)
    assert np.array_equal(got, want)
    if result is None:
        assert raised and sorted(set(e[2] for e in errors)) == [3, 6]  # column 5 is p3 of output column 3 and p0 of column 6
    else:
        assert not raised and not errors and (got[0, :5, 3] == result).all()  # (row 5 is outside: cval)


def test_trilinear_truncates_toward_zero(oracle):
    vol = tc.cast_volume(np.int16, -4, -4)
    vol[:, :, 4] = -3
    got, want, raised, errors = _both(oracle, vol, (1.0, 1.0, 1.0), tc.cast_matrix(), tc.CAST_N, "AXIAL", 1, -100, tc.CAST_OSHAPE)
    assert not raised and np.array_equal(got, want) and (got[0, :5, 3] == -3).all()  # -3.5 -> -3, not the floor -4


@pytest.mark.parametrize("shape", [(1, 6, 7), (5, 1, 7), (5, 6, 1)])
def test_axis_of_length_1_is_all_cval(oracle, shape):
    """0 <= n < d - 1 has no solution for d = 1: every mode returns cval everywhere and nothing is read"""
    vol = np.random.default_rng(5).integers(-900, 1000, shape).astype(np.int16)
    for m in (np.eye(4), tc.translation(2, 0.25, (1.0, 1.0, 1.0))):
        for minterpol in (0, 1, 2, 3):
            got, want, raised, errors = _both(oracle, vol, (1.0, 1.0, 1.0), m, 0, "OTHER", minterpol, -1000, shape)
            assert not raised and not errors and (got == -1000).all() and (want == -1000).all()


def _quarter_shift():
    m = np.eye(4)
    m[:3, 3] = 0.25
    return m


@pytest.mark.parametrize("shape", [(2, 6, 7), (5, 2, 7), (5, 6, 2), (3, 4, 5)])
def test_short_axes(oracle, shape):
    """length 2: nearest .. tricubic wrap inside the axis; Lanczos reaches tap -3 -> -1 -> panic for every inside voxel, cval there.
    (3, 4, 5) is the smallest volume on which Lanczos is legal."""
    vol = np.random.default_rng(6).integers(-900, 1000, shape).astype(np.int16)
    sp = (1.0, 1.0, 1.0)
    inside = tc.source_coords(shape, sp, _quarter_shift(), 0, "OTHER", shape)[3]
    assert inside.sum() == (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)
    for minterpol in (0, 1, 2, 3):
        got, want, raised, errors = _both(oracle, vol, sp, _quarter_shift(), 0, "OTHER", minterpol, -1000, shape)
        assert np.array_equal(got, want)
        if minterpol == 3 and 2 in shape:
            assert raised and sorted(errors) == sorted(map(tuple, np.argwhere(inside))) and (got == -1000).all()
        else:
            assert not raised and not errors and (got[inside] != -1000).all()
    if 2 in shape:  # every voxel mapped outside: the reference returns cval everywhere and never reaches the taps
        got, want, raised, errors = _both(oracle, vol, sp, tc.translation(1, 100, sp), 0, "OTHER", 3, -1000, shape)
        assert not raised and not errors and (got == -1000).all() and (want == -1000).all()


def _homogeneous(kind):
    m = tc.matrix()
    if kind == "w":
        m[3, 3] = 1.25
    elif kind == "row":
        m[3, :3] = (1e-3, -2e-3, 5e-4)
    else:
        m[3, :] = 0.0
    return m


@pytest.mark.parametrize("kind", ["w", "row", "zero"])
@pytest.mark.parametrize("minterpol", [0, 1, 2])
def test_homogeneous_rows(oracle, kind, minterpol):
    vol = tc.volume(np.int16)
    cval = int(vol.min())
    orientation, n, oshape = tc.OTHER
    got, want, raised, errors = _both(oracle, vol, tc.SPACING, _homogeneous(kind), n, orientation, minterpol, cval, oshape)
    assert not raised and not errors and np.array_equal(got, want)
    if kind == "zero":
        assert (got == cval).all()  # every coordinate is inf or NaN
    else:
        plain = np.zeros(oshape, np.int16)
        oracle.apply_view_matrix_transform(vol, tc.SPACING, tc.matrix(), n, orientation, minterpol, cval, plain)
        assert (got != cval).mean() > 0.3 and (got != plain).any()  # the row matters
