"""The indexed mesh of a marching-cubes piece restated with numpy (test infrastructure; imports nothing from the package): which
vertices csrc/k_mci.hip must produce, where, and IN WHICH ORDER.  A vertex is a grid edge of the padded, Y-flipped piece whose two
ends lie on different sides of the iso-value; when one end's sample EQUALS the iso-value the vertex sits on that grid point and all
such edges around the point share one "point vertex".  Ids follow the raster order of 64-point words (plane, row, word) and inside
a word x edges, y edges, z edges, point vertices, each by bit -- the order both sides of the cross-slab stitch count on.
tests/test_mci_cases_host.py checks this restatement against the C oracle's soup; tests/test_gpu_mci_edges.py holds the kernels
to it array for array."""
import numpy as np

KIND_X, KIND_Y, KIND_Z, KIND_POINT = 0, 1, 2, 3


def padded_grid(a, pad_xy, pad_bottom, pad_top, pad_value):
    """The padded point grid (NZ, NY, NX) float64 as mc_at reads it: the source at [pb:, pxy:, pxy:] with its y axis reversed (padded
    row jf holds source row (NY - 1 - jf) - pxy), `pad_value` elsewhere."""
    nz, ny, nx = a.shape
    pxy, pb, pt = int(bool(pad_xy)), int(bool(pad_bottom)), int(bool(pad_top))
    P = np.full((nz + pb + pt, ny + 2 * pxy, nx + 2 * pxy), float(pad_value), np.float64)
    P[pb:pb + nz, pxy:pxy + ny, pxy:pxy + nx] = a[:, ::-1, :]
    return P


def _sl(axis, lo):
    s = [slice(None)] * 3
    s[axis] = slice(None, -1) if lo else slice(1, None)
    return tuple(s)


def crossing_planes(P, iso):
    """(S, E, cross, point): inside plane, on-iso plane, per axis (z, y, x order of the ARRAY axes 0, 1, 2) the crossing edges as a
    boolean array at the edge's low end (False where the edge does not exist), and the points of E that are an end of some
    crossing edge -- in any of the six directions."""
    S, E = P >= iso, P == iso
    cross, point = [], np.zeros(P.shape, bool)
    for axis in range(3):
        c = np.zeros(P.shape, bool)
        if P.shape[axis] > 1:
            c[_sl(axis, True)] = S[_sl(axis, True)] != S[_sl(axis, False)]
        cross.append(c)
        point[_sl(axis, True)] |= c[_sl(axis, True)]      # the edge leaves its low end ...
        point[_sl(axis, False)] |= c[_sl(axis, True)]     # ... and arrives at its high end
    return S, E, cross, point & E


def indexed_vertices(a, spacing, iso, roi_start, pad_xy, pad_bottom, pad_top, pad_value, vtk_pz):
    """(verts float32 (V, 3), keys int64 (V, 5)) of ONE iso-value, sorted by key = (k, jf, i >> 6, kind, i & 63)."""
    P = padded_grid(a, pad_xy, pad_bottom, pad_top, pad_value)
    NZ, NY, NX = P.shape
    pxy = int(bool(pad_xy))
    yoff, zoff = NY - 1 - pxy, int(roi_start) - int(vtk_pz)
    iso = float(iso)
    if min(P.shape) < 2:  # no cell, no surface (mc_piece_layout: `empty`): crossing edges of such a grid belong to no triangle
        return np.zeros((0, 3), np.float32), np.zeros((0, 5), np.int64)
    _, E, cross, point = crossing_planes(P, iso)
    pos, keys = [], []
    # array axis 2 is x (kind 0), 1 is y (kind 1), 0 is z (kind 2); kind 3 are the point vertices
    for kind, axis in ((KIND_X, 2), (KIND_Y, 1), (KIND_Z, 0), (KIND_POINT, None)):
        if axis is None:
            sel, t = point, None
        else:
            sel = cross[axis].copy()
            sel[_sl(axis, True)] &= ~(E[_sl(axis, True)] | E[_sl(axis, False)])
            hi = np.zeros(P.shape, np.float64)
            hi[_sl(axis, True)] = P[_sl(axis, False)]
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (iso - P) / (hi - P)
        k, jf, i = np.nonzero(sel)
        p = [(i - pxy).astype(np.float64), (jf - yoff).astype(np.float64), (k + zoff).astype(np.float64)]
        if axis is not None:
            p[2 - axis] = p[2 - axis] + t[k, jf, i]
        pos.append(np.stack([np.float64(spacing[q]) * p[q] for q in range(3)], axis=1))
        keys.append(np.stack([k, jf, i >> 6, np.full(len(k), kind), i & 63], axis=1).astype(np.int64))
    pos, keys = np.concatenate(pos), np.concatenate(keys)
    order = np.lexsort(tuple(keys[:, c] for c in (4, 3, 2, 1, 0)))
    return pos[order].astype(np.float32), keys[order]


def _ranks(verts, corners):
    """one int64 per float32 triple, equal where the three bit patterns are: (keys of verts, keys of corners)"""
    both = np.concatenate([np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(corners, np.float32).reshape(-1, 3)])
    both = both.view(np.uint32)
    key = np.zeros(len(both), np.int64)
    for c in range(3):
        u, inv = np.unique(both[:, c], return_inverse=True)
        key = key * np.int64(len(u) + 1) + inv.reshape(-1)
    return key[:len(verts)], key[len(verts):]


def has_duplicates(verts):
    k, _ = _ranks(verts, np.zeros((0, 3), np.float32))
    return len(np.unique(k)) != len(k)


def lookup(verts, corners):
    """position of every corner (float32 triple, by bit pattern) in `verts`; raises if one is missing or verts has duplicates"""
    kv, kc = _ranks(verts, corners)
    order = np.argsort(kv, kind="stable")
    sk = kv[order]
    if len(sk) > 1 and np.any(sk[1:] == sk[:-1]):
        raise ValueError("duplicate vertices")
    if len(kc) == 0:
        return np.zeros(0, np.int64)
    if len(sk) == 0:
        raise ValueError("a soup vertex is not among the restated vertices")
    at = np.minimum(np.searchsorted(sk, kc), len(sk) - 1)
    if np.any(sk[at] != kc):
        raise ValueError("a soup vertex is not among the restated vertices")
    return order[at]


def indexed_mesh(a, args, soup):
    """(verts, faces int32 (T, 3)) for args = (spacing, iso_values, roi_start, pad_xy, pad_bottom, pad_top, pad_value, vtk_pz).
    `soup`: the oracle's (T, 3, 3) soup for one iso-value, or a list with one soup per iso-value (each iso-value has an id range of
    its own, iso 0's first, and the faces of iso q point into range q only)."""
    spacing, isos = args[0], list(args[1])
    soups = [soup] if isinstance(soup, np.ndarray) else list(soup)
    assert len(soups) == len(isos)
    vs, fs, base = [], [], 0
    for iso, s in zip(isos, soups):
        v, _ = indexed_vertices(a, spacing, iso, *args[2:])
        f = lookup(v, np.asarray(s, np.float32).reshape(-1, 3)).reshape(-1, 3) + base
        vs.append(v)
        fs.append(f)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def shared_plane_counts(lower_keys, upper_keys, NZ_lower):
    """how many vertices two neighbouring pieces both carry: the x edges, y edges and point vertices (kinds 0, 1, 3) of the lower
    piece's plane NZ_lower - 1, matched against the upper piece's plane 0 on (jf, word, kind, bit)"""
    lo = lower_keys[(lower_keys[:, 0] == NZ_lower - 1) & (lower_keys[:, 3] != KIND_Z)][:, 1:]
    up = upper_keys[(upper_keys[:, 0] == 0) & (upper_keys[:, 3] != KIND_Z)][:, 1:]
    return len(set(map(tuple, lo.tolist())) & set(map(tuple, up.tolist())))
