"""Test infrastructure for the geodesic measure: the mesh builders, the numpy / heapq restatement of the rules of
include/ivx.h and the path checker.  The distance field is the least fixed point of d[v] = min_u fl(d[u] + w(u, v)) over the
triangle sides, w = sqrt((dx dx + dy dy) + dz dz) in float64 from the float32 positions: scipy.sparse.csgraph.dijkstra, the
heapq Dijkstra and the synchronous relaxation below all give it bit for bit (tests/test_geodesic_host.py)."""
import heapq

import numpy as np


# ---- the rules ----
def edges(faces, nverts=None):
    """unique undirected pairs (a < b) of the triangle sides, no self edges, sorted: int64 (E, 2)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = e[e[:, 0] != e[:, 1]]
    e = np.sort(e, axis=1)
    return np.unique(e, axis=0) if len(e) else np.zeros((0, 2), np.int64)


def weights(verts, e):
    p = np.asarray(verts, np.float32).astype(np.float64)
    d = p[e[:, 0]] - p[e[:, 1]]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def csr(faces, nverts):
    """``(offsets uint32 (V + 1,), neighbours uint32)``: the unique neighbours of every point in ascending order"""
    e = edges(faces)
    both = np.concatenate([e, e[:, ::-1]])
    both = both[np.lexsort((both[:, 1], both[:, 0]))]
    off = np.zeros(nverts + 1, np.uint32)
    off[1:] = np.cumsum(np.bincount(both[:, 0], minlength=nverts))
    return off, both[:, 1].astype(np.uint32)


def scipy_dijkstra(verts, faces, source):
    """live scipy on the same graph; stored zero weights are edges in its CSR input"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    n = len(verts)
    e = edges(faces)
    w = weights(verts, e)
    m = csr_matrix((np.concatenate([w, w]), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))), shape=(n, n))
    return dijkstra(m, directed=True, indices=int(source))


def heap_dijkstra(verts, faces, source):
    """``(dist float64, pred int64)`` by a heapq Dijkstra; pred -1 at the source and where it does not reach"""
    n = len(verts)
    e = edges(faces)
    w = weights(verts, e)
    nb = [[] for _ in range(n)]
    for (a, b), x in zip(e.tolist(), w.tolist()):
        nb[a].append((b, x))
        nb[b].append((a, x))
    dist, pred = np.full(n, np.inf), np.full(n, -1, np.int64)
    dist[source] = 0.0
    done = np.zeros(n, bool)
    heap = [(0.0, int(source))]
    while heap:
        d, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        for v, x in nb[u]:
            c = d + x
            if c < dist[v]:
                dist[v], pred[v] = c, u
                heapq.heappush(heap, (c, v))
    return dist, pred


def bellman_ford(verts, faces, source):
    """the synchronous relaxation in numpy, to its fixed point"""
    n = len(verts)
    e = edges(faces)
    w = weights(verts, e)
    a, b, w = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]), np.concatenate([w, w])
    dist = np.full(n, np.inf)
    dist[source] = 0.0
    for _ in range(4 * n + 64):
        new = dist.copy()
        np.minimum.at(new, b, dist[a] + w)
        if np.array_equal(new, dist):
            return dist
        dist = new
    raise AssertionError("no fixed point")


def check_path(verts, faces, ids, start, end, d_end):
    """`ids` is a path from `start` to `end` along triangle sides that visits no point twice, and the float64 running sum of its
    edge lengths from the start equals `d_end` exactly"""
    ids = [int(i) for i in ids]
    assert len(ids) >= 1 and ids[0] == int(start) and ids[-1] == int(end), (ids[:3], ids[-3:], start, end)
    assert len(set(ids)) == len(ids), "a point repeats"
    have = set(map(tuple, edges(faces).tolist()))
    p = np.asarray(verts, np.float32).astype(np.float64)
    total = np.float64(0.0)
    for a, b in zip(ids[:-1], ids[1:]):
        assert (min(a, b), max(a, b)) in have, "no triangle side joins %d and %d" % (a, b)
        d = p[a] - p[b]
        total = total + np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    assert total == d_end, (float(total), float(d_end))


# ---- the meshes ----
def grid(nx, ny, jitter=0.0, seed=7, shift=(0.0, 0.0, 0.0)):
    """an nx x ny grid of points (id = y * nx + x), two triangles per cell"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:ny, :nx]
    v = np.stack([x.ravel(), y.ravel(), np.zeros(nx * ny)], 1).astype(np.float64)
    if jitter:
        v += rng.uniform(-jitter, jitter, v.shape)
    v += np.asarray(shift, np.float64)
    i = (y[:-1, :-1] * nx + x[:-1, :-1]).ravel()
    f = np.concatenate([np.stack([i, i + 1, i + nx], 1), np.stack([i + 1, i + nx + 1, i + nx], 1)])
    return v.astype(np.float32), f.astype(np.int32)


def strip(n):
    """n points in two rows (ids alternate between the rows), n - 2 triangles"""
    k = np.arange(n)
    v = np.stack([(k // 2) * 1.0 + 0.25 * (k % 2), (k % 2) * 0.75, 0.1 * np.sin(k * 0.37)], 1)
    f = np.stack([k[:-2], k[1:-1], k[2:]], 1)
    return v.astype(np.float32), f.astype(np.int32)


def strip2(cols):
    """a 2 x cols strip: row 0 holds ids 0 .. cols-1, row 1 the rest"""
    return grid(cols, 2, jitter=0.2, seed=11)


def jittered_grid(shift=(0.0, 0.0, 0.0)):
    """the 40 x 41 grid (1 640 points) with two pairs of coincident points joined by an edge"""
    v, f = grid(40, 41, jitter=0.3, seed=3)
    v[40 * 10 + 11] = v[40 * 10 + 10]  # horizontal neighbours
    v[40 * 31 + 25] = v[40 * 30 + 25]  # vertical neighbours
    return (v.astype(np.float64) + np.asarray(shift, np.float64)).astype(np.float32), f


def fan(n=300):
    """n triangles around hub 0; rim ids 1 .. n, closed"""
    a = np.arange(n) * (2 * np.pi / n)
    v = np.concatenate([[[0.0, 0.0, 0.5]], np.stack([np.cos(a) * (2 + 0.3 * np.sin(5 * a)), np.sin(a) * 2, np.zeros(n)], 1)])
    r = np.arange(1, n + 1)
    f = np.stack([np.zeros(n, np.int64), r, np.roll(r, -1)], 1)
    return v.astype(np.float32), f.astype(np.int32)


def two_blobs(n=48):
    """the uint8 volume of two separate balls, for the project's own marching cubes"""
    z, y, x = np.mgrid[:n, :n, :n]
    m = np.zeros((n, n, n), np.uint8)
    m[(z - 24) ** 2 + (y - 24) ** 2 + (x - 15) ** 2 <= 11 ** 2] = 255
    m[(z - 24) ** 2 + (y - 22) ** 2 + (x - 37) ** 2 <= 6 ** 2] = 255
    return m
