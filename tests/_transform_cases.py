"""Shared inputs of the view-matrix resampler tests (tests/test_gpu_transform_edges.py on the GPU,
tests/test_oracle_transform.py on the CPU): one small ramp volume in the three dtypes, one real matrix, the four
placements, the cast-bound profiles, and a float64 numpy restatement of coord_transform's coordinates
(transforms.rs:21-31) that says which output voxels fall inside and how large a Lanczos-4 sum's terms are.

The volume is a ramp plus a little noise: the wrap-around of get_value (interpolation.rs:6-35) is then a large step, and
every tap stays distinguishable from its neighbours."""
import numpy as np

SHAPE = (9, 11, 13)
SPACING = (0.5, 0.75, 2.0)  # (sx, sy, sz)
PLACEMENTS = [("AXIAL", 3, (3, 11, 13)), ("CORONAL", 4, (9, 3, 13)), ("SAGITAL", 5, (9, 11, 3)), ("OTHER", 0, (9, 11, 13))]
OTHER = PLACEMENTS[3]
DTYPES = [np.uint8, np.int16, np.float64]
EPS = float(np.finfo(np.float64).eps)


def rot(shape, spacing, angles):
    """T(c) R T(-c) about the volume centre in (z, y, x) world coordinates, like slice_.py:1977-1978"""
    az, ay, ax = angles
    cz, sz_ = np.cos(az), np.sin(az)
    cy, sy_ = np.cos(ay), np.sin(ay)
    cx, sx_ = np.cos(ax), np.sin(ax)
    Rz = np.array([[1, 0, 0], [0, cz, -sz_], [0, sz_, cz]])
    Ry = np.array([[cy, 0, sy_], [0, 1, 0], [-sy_, 0, cy]])
    Rx = np.array([[cx, -sx_, 0], [sx_, cx, 0], [0, 0, 1]])
    R = np.eye(4)
    R[:3, :3] = Rz @ Ry @ Rx
    c = np.array([shape[0] * spacing[2], shape[1] * spacing[1], shape[2] * spacing[0]]) / 2.0
    T0, T1 = np.eye(4), np.eye(4)
    T0[:3, 3] = -c
    T1[:3, 3] = c
    return np.ascontiguousarray(T1 @ R @ T0)


def base_volume():
    """40 + 9z + 5y + 4x + noise in 0..11: within 40 .. 221, so it is a uint8 volume as it stands"""
    rng = np.random.default_rng(3)
    z, y, x = np.meshgrid(np.arange(SHAPE[0]), np.arange(SHAPE[1]), np.arange(SHAPE[2]), indexing="ij")
    b = 40 + 9 * z + 5 * y + 4 * x + rng.integers(0, 12, SHAPE)
    assert b.min() >= 40 and b.max() <= 221
    return b


def volume(dtype):
    b = base_volume()
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return b.astype(np.uint8)
    if dtype == np.int16:
        return (b * 40 - 4000).astype(np.int16)
    return b.astype(np.float64) * 0.37 + 0.001


def matrix():
    """a rotation about the volume centre plus a nudge in world units"""
    M = rot(SHAPE, SPACING, (0.15, -0.1, 0.2))
    M[:3, 3] += (0.3, -0.2, 0.1)
    return np.ascontiguousarray(M)


def translation(axis, voxels, spacing):
    """out[c] samples vol[c + voxels] along `axis` (0 z, 1 y, 2 x): the offset in world units of that axis"""
    M = np.eye(4)
    M[axis, 3] = voxels * (spacing[2], spacing[1], spacing[0])[axis]
    return M


def run(fn, vol, spacing, M, n, orientation, minterpol, cval, oshape, fill=0):
    out = np.full(oshape, fill, vol.dtype)
    fn(vol, spacing, M, n, orientation, minterpol, cval, out)
    return out


def source_coords(vshape, spacing, M, n, orientation, oshape):
    """(nz, ny, nx, inside) of every output voxel: transforms.rs:21-31 in float64 numpy, the reference's operation order"""
    sx, sy, sz = (float(s) for s in spacing)
    z, y, x = (a.astype(np.float64) for a in np.meshgrid(np.arange(oshape[0]), np.arange(oshape[1]), np.arange(oshape[2]), indexing="ij"))
    if orientation == "AXIAL":
        z = z + n
    elif orientation == "CORONAL":
        y = y + n
    elif orientation == "SAGITAL":
        x = x + n
    c0, c1, c2 = z * sz, y * sy, x * sx
    m = np.asarray(M, np.float64)
    with np.errstate(all="ignore"):
        nc = [((m[r, 0] * c0 + m[r, 1] * c1) + m[r, 2] * c2) + m[r, 3] * 1.0 for r in range(4)]
        nz, ny, nx = (nc[0] / nc[3]) / sz, (nc[1] / nc[3]) / sy, (nc[2] / nc[3]) / sx
        dz, dy, dx = (float(d) for d in vshape)
        inside = (nz >= 0.0) & (nz < dz - 1.0) & (ny >= 0.0) & (ny < dy - 1.0) & (nx >= 0.0) & (nx < dx - 1.0)
    return nz, ny, nx, inside


def _lanczos_k(x, a=4.0):
    """interpolation.rs:55-64, vectorised"""
    safe = np.where(x == 0.0, 1.0, x)
    k = (a * np.sin(np.pi * safe) * np.sin(np.pi * (safe / a))) / (np.pi * np.pi * safe * safe)
    return np.where(x == 0.0, 1.0, np.where((-a <= x) & (x < a), k, 0.0))


def _taps(coord, d):
    f = np.floor(coord).astype(np.int64)
    i = f[:, None] + np.arange(-3, 4)[None, :]
    k = _lanczos_k(coord[:, None] - i.astype(np.float64))
    i = np.where(i < 0, i + d, np.where(i >= d, i - d, i))  # one wrap per axis
    assert i.min() >= 0 and i.max() < d, "a Lanczos tap leaves the axis after one wrap"
    return i, k


def lanczos_abs_sum(vol, spacing, M, n, orientation, oshape):
    """S = sum |v_ijk kx_i ky_j kz_k| over the 343 taps of every inside voxel (0 outside), float64: the scale against which a
    Lanczos result's rounding is measured.  Returns (S, inside)."""
    nz, ny, nx, inside = source_coords(vol.shape, spacing, M, n, orientation, oshape)
    S = np.zeros(oshape, np.float64)
    sel = np.nonzero(inside.ravel())[0]
    if sel.size:
        iz, kz = _taps(nz.ravel()[sel], vol.shape[0])
        iy, ky = _taps(ny.ravel()[sel], vol.shape[1])
        ix, kx = _taps(nx.ravel()[sel], vol.shape[2])
        v = np.abs(vol[iz[:, :, None, None], iy[:, None, :, None], ix[:, None, None, :]].astype(np.float64))
        S.ravel()[sel] = np.einsum("nkji,nk,nj,ni->n", v, np.abs(kz), np.abs(ky), np.abs(kx))
    return S, inside


def one_lsb(g, r):
    """the rule for Lanczos on integer dtypes: within 1 LSB everywhere, on at most max(1, 1e-3 N) voxels"""
    d = np.abs(g.astype(np.int64) - r.astype(np.int64))
    return int(d.max()), int((d > 0).sum()), max(1, int(1e-3 * d.size))


# ---- cast bounds: tricubic at half a voxel along x -------------------------------------------------------------------
# Volume (6, 6, 8), every row the constant `c` with column 5 set to `p3`; identity with M[2, 3] = 0.5, spacing 1, AXIAL n = 2,
# output (1, 6, 8).  Output column 3 samples x = 3.5 from columns 2..5: (-c + 9c + 9c - p3) / 16, exact in double (all the
# intermediate values of cubic_interpolate are multiples of 1/16 below 2^24).  Column 6 reads column 5 as p0 (the same
# value); columns 4 and 5 see it as p2 / p1 and move the other way, towards the inside of the range.
CAST_SHAPE, CAST_OSHAPE, CAST_N = (6, 6, 8), (1, 6, 8), 2
CAST_PROFILES = [  # dtype, c, p3, value at x = 3.5, result (None: NumCast fails -> ValueError)
    (np.int16, -32768, -32762, -32768.375, -32768),
    (np.int16, -32768, -32750, -32769.125, None),
    (np.int16, 32767, 32761, 32767.375, 32767),
    (np.int16, 32767, 32750, 32768.0625, None),
    (np.uint8, 0, 6, -0.375, 0),
    (np.uint8, 0, 17, -1.0625, None),
    (np.uint8, 255, 249, 255.375, 255),
    (np.uint8, 255, 238, 256.0625, None),
]


def cast_matrix():
    M = np.eye(4)
    M[2, 3] = 0.5
    return M


def cast_volume(dtype, c, p3):
    v = np.full(CAST_SHAPE, c, dtype)
    v[:, :, 5] = p3
    return v
