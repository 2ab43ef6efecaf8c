"""The surface connectivity rules of DESIGN 7h restated with numpy + scipy (the checker of tests/test_gpu_mesh_regions.py; VTK is
not installed, so this -- not VTK -- is what the kernels are pinned against):

* regions are the connected components of the graph whose nodes are point ids and whose edges join the corners of a triangle;
  a point no triangle uses belongs to no region (label -1);
* region r is the r-th region in ascending order of its first (smallest-index) triangle;
* part r = the triangles labelled r in their original order, on the points they use in original order, ids remapped;
* seeded = the union of the regions that hold a seed point, as triangles in order, then points compacted in order;
* largest = most triangles, the lowest r on a tie."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def region_labels(nverts, faces):
    """-> (tri_labels int32 (T,), vert_labels int32 (V,), n_regions)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return np.zeros(0, np.int32), np.full(nverts, -1, np.int32), 0
    rows = np.concatenate([f[:, 0], f[:, 0]])
    cols = np.concatenate([f[:, 1], f[:, 2]])
    g = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(nverts, nverts))
    _, comp = connected_components(g, directed=False)
    tcomp = comp[f[:, 0]]
    first = np.full(comp.max() + 1, len(f), np.int64)       # first triangle of every component (len(f): has none)
    np.minimum.at(first, tcomp, np.arange(len(f)))
    order = np.argsort(first, kind="stable")                # components by first triangle; those without one come last
    n = int(np.count_nonzero(first < len(f)))
    rank = np.full(len(first), -1, np.int64)
    rank[order[:n]] = np.arange(n)
    return rank[tcomp].astype(np.int32), rank[comp].astype(np.int32), n


def compact(verts, faces, keep):
    """the triangles with keep[t], in order, on the points they use, compacted in order"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)[np.asarray(keep, bool)]
    used = np.zeros(len(v), bool)
    used[f.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return v[used], new[f].astype(np.int32).reshape(-1, 3)


def split(verts, faces):
    """-> (list of (verts, faces) in region order, table int64 (R, 4) = (tri offset, ntris, vert offset, nverts))"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    tl, _, n = region_labels(len(v), faces)
    order = np.argsort(tl, kind="stable")
    counts = np.bincount(tl, minlength=n)
    parts, table, to, vo = [], np.zeros((n, 4), np.int64), 0, 0
    start = np.concatenate([[0], np.cumsum(counts)])
    keep = np.zeros(len(tl), bool)
    for r in range(n):
        keep[:] = False
        keep[order[start[r]:start[r + 1]]] = True
        pv, pf = compact(v, faces, keep)
        parts.append((pv, pf))
        table[r] = (to, len(pf), vo, len(pv))
        to, vo = to + len(pf), vo + len(pv)
    return parts, table


def split_grouped(verts, faces):
    """the same split without a loop over the parts: (grouped verts, grouped faces with part-local ids, table)"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    tl, vl, n = region_labels(len(v), f)
    order_t = np.argsort(tl, kind="stable")
    order_v = np.argsort(np.where(vl < 0, n, vl), kind="stable")[:int(np.count_nonzero(vl >= 0))]
    tcount, vcount = np.bincount(tl, minlength=n)[:n], np.bincount(vl[order_v], minlength=n)[:n]
    toff, voff = np.cumsum(tcount) - tcount, np.cumsum(vcount) - vcount
    new = np.full(len(v), -1, np.int64)
    new[order_v] = np.arange(len(order_v)) - voff[vl[order_v]]
    table = np.stack([toff, tcount, voff, vcount], axis=1).astype(np.int64).reshape(n, 4)
    return v[order_v], new[f[order_t]].astype(np.int32).reshape(-1, 3), table


def seeded(verts, faces, ids):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    tl, vl, n = region_labels(len(v), faces)
    want = np.zeros(n + 1, bool)
    want[vl[np.asarray(ids, np.int64).reshape(-1)]] = True  # (-1, an unused point, lands in the spare slot)
    want[n] = False
    return compact(v, faces, want[tl])


def largest(verts, faces):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    tl, _, n = region_labels(len(v), faces)
    if n == 0:
        return compact(v, faces, np.zeros(len(tl), bool))
    return compact(v, faces, tl == int(np.argmax(np.bincount(tl, minlength=n))))  # argmax: the first among equals


def nearest_point(verts, xyz):
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    if len(v) == 0:
        return -1
    d = v - np.asarray(xyz, np.float64)
    return int(np.argmin((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))  # argmin: the first among equals


# ---- the hand-numbered mesh of the tests: 12 points, 10 triangles, 4 regions --------------------------------------------------
#   region 0: triangles 0 and 5, which share ONE point (2)                 points 0 1 2 3 4
#   region 1: triangles 1, 3, 7: a strip                                    points 5 6 7 8 (triangle 7 repeats point 8)
#   region 2: triangles 2, 4, 8: as large as region 1 (the tie)            points 10 11 12 13 14
#   region 3: triangles 6, 9                                                points 15 16 17 18
#   point 9 is used by no triangle
HAND_FACES = np.array([[0, 1, 2], [5, 6, 7], [10, 11, 12], [6, 7, 8], [11, 12, 13], [2, 3, 4], [15, 16, 17], [7, 8, 8], [12, 13, 14],
                       [16, 17, 18]], np.int32)
HAND_TRI_LABELS = np.array([0, 1, 2, 1, 2, 0, 3, 1, 2, 3], np.int32)
HAND_VERT_LABELS = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1, -1, 2, 2, 2, 2, 2, 3, 3, 3, 3], np.int32)
HAND_TABLE = np.array([[0, 2, 0, 5], [2, 3, 5, 4], [5, 3, 9, 5], [8, 2, 14, 4]], np.int64)


def hand_mesh():
    rng = np.random.default_rng(5)
    return rng.standard_normal((19, 3)).astype(np.float32), HAND_FACES.copy()
