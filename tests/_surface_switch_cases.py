"""Test infrastructure (imports nothing from the package): the meshes that put the surface tail's kernels -- csrc/k_smooth.hip,
k_meshtail.hip, k_meshgeo.hip, k_mesh.hip with mesh_regions.h and scan_u32.h -- on either side of every switch between two code
paths, and the constants of those switches, restated.  tests/test_surface_switch_cases_host.py checks, without a GPU, that the
constants are the ones the .hip / .h text defines and that every case sits on the side it is named for;
tests/test_gpu_surface_switches.py runs the kernels on them.  Every builder is seeded, and every coordinate is jittered so that
no two sums are symmetric by accident (`tie_strip` and the placements with exact distances say so where they are not)."""
import numpy as np

# ---- the switches, restated (test_surface_switch_cases_host.py matches each against the source text) ----
RL = 12                    # k_smooth.hip: incident faces / unique neighbours of a vertex kept in registers
FAN_LANE_MAX = 48          # k_meshtail.hip: corners of a vertex sorted by one lane; beyond that by a workgroup
RIM_TURNS = 64             # k_meshtail.hip: faces turned through about a rim vertex before the chain is given up
GEO_INSERTION_MAX = 32     # k_meshgeo.hip: raw neighbour list sorted by insertion; beyond that by heap sort
TRICOUNT_BLOCK = 2048      # mesh_regions.h: triangles per workgroup of k_mesh_tricount (256 lanes x TPL 8)
MASS_BLOCK = 1024          # k_mesh.hip: triangles per workgroup of k_mesh_mass (256 lanes x MASS_TPL 4)
MASS_FINAL_LANES = 256     # k_mesh.hip: partial records k_mesh_mass_final takes per trip of its strided loop
SCAN_BLOCK = 4096          # scan_u32.h: elements per workgroup of k_mscan_block (256 lanes x MSCAN 16)
SCAN_SUMS_PASS = 1024      # scan_u32.h: block sums per pass of k_mscan_sums
HASH_MIN_SLOTS = 1024      # k_meshtail.hip: the edge hash's smallest table
BIG_SORT_GRID = 1024       # k_meshtail.hip: workgroups of k_fan_sort_big at the most

HUB_IDS = (0, 3, "last")   # vertex 3 is the Q-M1 vertex of the smoothing (oracle/ivx_oracle_mesh.c)


# ---- fans around a hub ----
def _renumber(verts, faces, hub_id):
    """the mesh with old vertex 0 (the hub) at id `hub_id` (0, 3 or "last"): the two ids change places"""
    n = len(verts)
    h = n - 1 if hub_id == "last" else int(hub_id)
    assert 0 <= h < n
    perm = np.arange(n)      # old id -> new id
    perm[0], perm[h] = h, 0
    out = np.empty_like(verts)
    out[perm] = verts
    return out, perm[faces].astype(np.int32), h


def _fan_points(n_rim, seed, dtype):
    rng = np.random.default_rng(seed)
    ang = (np.arange(n_rim) + rng.uniform(-0.2, 0.2, n_rim)) * (2 * np.pi / n_rim)
    rad = 1.0 + rng.uniform(-0.15, 0.15, n_rim)
    rim = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-0.1, 0.1, n_rim)], axis=1)
    hub = np.array([[0.03, -0.02, 0.3]]) + rng.uniform(-0.01, 0.01, (1, 3))
    return np.concatenate([hub, rim]).astype(dtype), rng


def closed_fan(k, hub_id=0, seed=0, dtype=np.float64):
    """k triangles around a hub, closed: k incident faces, k neighbours.  -> (verts, faces int32 (k, 3), hub)"""
    v, rng = _fan_points(k, seed, dtype)
    f = np.array([[0, 1 + i, 1 + (i + 1) % k] for i in rng.permutation(k)], np.int32)  # scrambled: the hub meets its neighbours in that order
    return _renumber(v, f, hub_id)


def open_fan(k, hub_id=0, seed=0, dtype=np.float64):
    """k triangles around a hub, one gap: k incident faces, k + 1 neighbours, the hub on the rim with k faces between its two
    rim edges.  The points cover 300 degrees, so that the rim is a simple polygon."""
    v, rng = _fan_points(k + 1, seed, dtype)
    ang = np.arange(k + 1) * (np.deg2rad(300.0) / k)
    rad = np.hypot(v[1:, 0], v[1:, 1]).astype(np.float64)
    v[1:, 0], v[1:, 1] = rad * np.cos(ang), rad * np.sin(ang)
    f = np.array([[0, 1 + i, 2 + i] for i in rng.permutation(k)], np.int32)
    return _renumber(v, f, hub_id)


def bowtie(k, hub_id=0, seed=0, dtype=np.float64):
    """k triangles that share the hub and nothing else: k incident faces, 2 k neighbours"""
    v, rng = _fan_points(2 * k, seed, dtype)
    f = np.array([[0, 1 + 2 * i, 2 + 2 * i] for i in rng.permutation(k)], np.int32)
    return _renumber(v, f, hub_id)


FANS = {"closed": closed_fan, "open": open_fan, "bowtie": bowtie}
# (builder, k): 11 / 12 / 13 incident faces stand on either side of RL; bowtie(6) has exactly RL neighbours from 6 faces, bowtie(7),
# open_fan(12) and bowtie(11 / 12) have more than RL neighbours from at most RL register-sorted faces (the mixed path)
FAN_LADDER = [(name, k) for name in ("closed", "open", "bowtie") for k in (11, 12, 13)] + [("bowtie", 6), ("bowtie", 7)]


def with_repeat(verts, faces, hub, kind):
    """the fan with one face more: "degenerate" appends [hub, hub, a] (listed twice at the hub), "duplicate" an exact copy of a fan
    triangle (two face ids, the same three points)"""
    first = faces[0]
    a = int(first[first != hub][0])
    extra = [hub, hub, a] if kind == "degenerate" else first.tolist()
    return verts, np.concatenate([faces, np.array([extra], np.int32)]), hub


def reversed_faces(faces):
    """the same triangles listed in the opposite order: every vertex meets its neighbours the other way round"""
    return np.ascontiguousarray(faces[::-1])


def faces4(faces):
    f4 = np.empty((len(faces), 4), np.int64)
    f4[:, 0] = 3
    f4[:, 1:] = faces
    return f4


# ---- propagate_weights: the tie and the edge of tmax ----
def tie_strip(small_id_side="far"):
    """A strip of seven triangles between two rows of points, mirror-symmetric about the plane x = 0 in coordinates that are
    multiples of 1/4: the two end points of the lower row are the seeds, and the middle point M = (0, 0, 0) hears from both in the
    same round at the same squared distance 4.  One triangle (M, D1, D2) hangs off M; D1 and D2 touch nothing else and lie at
    x > 0, so their squared distances to the two seeds differ -- their weights tell which seed M kept.  The seed at x = -2 (the
    far one from D1, D2) has the smaller id with "far", the larger with "near".
    -> (verts float64, faces, seed flags uint8, info) with info = dict(seeds=(left id, right id), mid=, dangling=(D1 id, D2 id))"""
    low = [(-2.0, 0.0), (-1.0, 0.0), (0.0, 0.0), (1.0, 0.0), (2.0, 0.0)]
    top = [(-1.5, 1.0), (-0.5, 1.0), (0.5, 1.0), (1.5, 1.0)]
    dang = [(0.25, -1.0), (0.75, -1.5)]
    pts = np.array([(x, y, 0.0) for x, y in low + top + dang])
    b, t, d = [0, 1, 2, 3, 4], [5, 6, 7, 8], [9, 10]
    f = []
    for i in range(4):
        f.append([b[i], b[i + 1], t[i]])
        if i < 3:
            f.append([t[i], b[i + 1], t[i + 1]])
    f.append([b[2], d[0], d[1]])
    f = np.array(f, np.int64)
    # ids: left seed and right seed get 1 and 9 (or 9 and 1); every other point keeps its place among the rest
    left, right = (1, 9) if small_id_side == "far" else (9, 1)
    rest = [i for i in range(len(pts)) if i not in (left, right)]
    perm = np.empty(len(pts), np.int64)
    perm[b[0]], perm[b[4]] = left, right
    perm[[i for i in range(len(pts)) if i not in (b[0], b[4])]] = rest
    verts = np.empty_like(pts)
    verts[perm] = pts
    faces = perm[f].astype(np.int32)
    seeds = np.zeros(len(pts), np.uint8)
    seeds[[left, right]] = 1
    return verts, faces, seeds, dict(seeds=(left, right), mid=int(perm[b[2]]), dangling=(int(perm[d[0]]), int(perm[d[1]])))


def weight_of(d_sq, tmax, bmin):
    """propagate_weights' last line (mesh.rs:282-286) for one squared distance"""
    return (1.0 - np.sqrt(np.float64(d_sq)) / tmax) * (1.0 - bmin) + bmin


def edge_345():
    """S = (0, 0, 0) is the seed; P = (3, 4, 0) is its neighbour at squared distance exactly 25; Q = (0, 6, 0), the third point of
    their triangle, is farther.  C and E hang behind P (triangle P, C, E) and are reached through P alone: with tmax = 5.0 the
    test d_sq > tmax^2 lets P in and C, E get weights above bmin; with the next double below 5.0 nothing but S is reached.
    -> (verts float64, faces, seed flags, ids dict)"""
    v = np.array([[0, 0, 0], [3, 4, 0], [0, 6, 0], [1, 2, 0], [2, 0, 0]], np.float64)
    f = np.array([[0, 1, 2], [1, 3, 4]], np.int32)
    s = np.zeros(5, np.uint8)
    s[0] = 1
    return v, f, s, dict(S=0, P=1, Q=2, C=3, E=4)


# ---- cones: hole filling and point normals ----
def cone(m, zig=0.4, seed=0, centre=(0.0, 0.0, 0.0), radius=10.0, height=6.0):
    """an apex (id 0) over an m-gon rim (ids 1 .. m) whose z alternates +zig, -zig (jittered by a fifth of it), open below:
    m triangles, one rim of m edges.  Filled, the cap's centroid has m corners like the apex; the zigzag folds the cap, so at a
    small feature angle it falls into many fans.  -> (verts float32, faces int32)"""
    rng = np.random.default_rng(seed)
    ang = (np.arange(m) + rng.uniform(-0.1, 0.1, m)) * (2 * np.pi / m)
    z = np.where(np.arange(m) % 2 == 0, zig, -zig) * (1.0 + rng.uniform(-0.2, 0.2, m))
    rim = np.stack([radius * np.cos(ang), radius * np.sin(ang), z], axis=1)
    apex = np.array([[0.1, -0.2, height]]) + rng.uniform(-0.05, 0.05, (1, 3))
    v = (np.concatenate([apex, rim]) + np.asarray(centre, np.float64)).astype(np.float32)
    r = np.arange(1, m + 1)
    f = np.stack([np.zeros(m, np.int64), r, np.roll(r, -1)], axis=1)
    return v, f[rng.permutation(m)].astype(np.int32)


def cones(count, m, zig=0.4, seed=0):
    """`count` separate cones over m-gons on a square grid, cone after cone"""
    vs, fs, base = [], [], 0
    side = int(np.ceil(np.sqrt(count)))
    for i in range(count):
        mi = m[i] if np.ndim(m) else m
        v, f = cone(mi, zig, seed + i, centre=(25.0 * (i % side), 25.0 * (i // side), 0.0))
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def pyramid_6x8():
    """four triangles over the rectangle 6 x 8 at z = 0: the rim's bounding box has the diagonal 10, its bounding sphere the radius
    5.0 exactly"""
    v = np.array([[0, 0, 0], [6, 0, 0], [6, 8, 0], [0, 8, 0], [3, 4, 5]], np.float32)
    f = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], np.int32)
    return v, f


def sheet(nt, seed=0):
    """an open sheet of nt triangles (3 nt directed edges): a strip between two jittered rows of points"""
    rng = np.random.default_rng(seed)
    k = np.arange(nt + 2)
    v = np.stack([(k // 2) * 1.0 + 0.25 * (k % 2), (k % 2) * 0.75, 0.1 * np.sin(k * 0.37)], axis=1) + rng.uniform(-0.05, 0.05, (nt + 2, 3))
    f = np.stack([k[:-2], k[1:-1], k[2:]], axis=1)
    f[1::2] = f[1::2, ::-1]  # every other triangle turned: one orientation all along
    return v.astype(np.float32), f.astype(np.int32)


# ---- strips: keep-largest ----
def strips(sizes, order="shuffled", seed=0, spare=3, permute_points=True):
    """disjoint triangle strips of the given sizes (strip s has sizes[s] triangles on sizes[s] + 2 points), `spare` unused points,
    point ids permuted.  Face order: "sorted" lists strip after strip, "shuffled" mixes all triangles, "round_robin" deals the
    triangles of all strips but the last one in turn (one of each strip, then the next of each ...) and lists the last strip after
    them.  -> (verts float32, faces int32, strip of every triangle)"""
    rng = np.random.default_rng(seed)
    faces, owner, base = [], [], 0
    for s, n in enumerate(sizes):
        i = np.arange(n, dtype=np.int64) + base
        faces.append(np.stack([i, i + 1, i + 2], axis=1))
        owner.append(np.full(n, s))
        base += n + 2
    f, owner = np.concatenate(faces), np.concatenate(owner)
    nv = base + spare
    if order == "shuffled":
        at = rng.permutation(len(f))
    elif order == "round_robin":
        last = len(sizes) - 1
        within = np.concatenate([np.arange(n) for n in sizes])
        key = np.where(owner == last, np.iinfo(np.int64).max, within)
        at = np.lexsort((owner, key))  # by turn, then by strip; the last strip's triangles after all others, in their order
    else:
        assert order == "sorted"
        at = np.arange(len(f))
    f, owner = f[at], owner[at]
    if permute_points:
        f = rng.permutation(nv)[f]
    return rng.standard_normal((nv, 3)).astype(np.float32), f.astype(np.int32), owner


# triangles of the larger strip next to a 5-triangle strip, no spare points (T = big + 5 triangles, V = big + 9 points): a strip on
# 4095 / 4096 / 4097 points, then the scan over the kept triangles (T + 1 entries) and the one over the used points (V + 1 entries)
# at 4095 / 4096 / 4097 (/ 4098) entries each
SCAN_CASES = [4093, 4094, 4095] + [SCAN_BLOCK + d - 6 for d in (-1, 0, 1)] + [SCAN_BLOCK + d - 10 for d in (-1, 0, 1, 2)]


def with_leading_triangle(verts, faces, owner):
    """the mesh with one triangle more, on three points of its own, listed FIRST: a region that owns triangle 0 and nothing else"""
    n = len(verts)
    rng = np.random.default_rng(n)
    v = np.concatenate([verts, rng.standard_normal((3, 3)).astype(np.float32)])
    f = np.concatenate([np.array([[n, n + 1, n + 2]], np.int32), faces])
    return v, f, np.concatenate([[owner.max() + 1], owner])


def carry_strips(nv=SCAN_SUMS_PASS * SCAN_BLOCK + SCAN_BLOCK + 1, lo=4193000, nbig=2100, nsmall=40):
    """4 198 401 points of which two strips use a few: the larger on point ids lo .. lo + nbig + 1, across element
    SCAN_SUMS_PASS * SCAN_BLOCK = 4 194 304 of the scan over the used points, the smaller from id 5.  The smaller strip's
    triangles come first.  -> (verts float32, faces int32)"""
    rng = np.random.default_rng(7)
    assert lo < SCAN_SUMS_PASS * SCAN_BLOCK < lo + nbig and lo + nbig + 2 <= nv
    i, j = np.arange(nsmall) + 5, np.arange(nbig) + lo
    f = np.concatenate([np.stack([i, i + 1, i + 2], axis=1), np.stack([j, j + 1, j + 2], axis=1)])
    v = np.zeros((nv, 3), np.float32)
    used = np.unique(f)
    v[used] = rng.standard_normal((len(used), 3))
    return v, f.astype(np.int32)


# ---- mass properties ----
def soup(nt, seed=0):
    """nt well-shaped triangles (T, 3, 3) float32: every triangle a jittered equilateral one of side ~1, turned at random, its
    centre up to 50 away from the origin"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 2 * np.pi, nt)[:, None] + np.array([0.0, 2 * np.pi / 3, 4 * np.pi / 3])
    flat = np.stack([np.cos(a), np.sin(a), np.zeros_like(a)], axis=2) * 0.6 + rng.uniform(-0.12, 0.12, (nt, 3, 3))
    q = rng.standard_normal((nt, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    rot = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                    np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                    np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)
    t = np.einsum("tij,tkj->tki", rot, flat) + rng.uniform(-50, 50, (nt, 1, 3))
    return t.astype(np.float32)


def indexed(tris, seed=0):
    """the same triangles as an indexed mesh: every corner its own point, the points in a permuted order"""
    rng = np.random.default_rng(seed)
    n = 3 * len(tris)
    perm = rng.permutation(n)
    v = np.empty((n, 3), np.float32)
    v[perm] = tris.reshape(-1, 3)
    return v, perm.reshape(-1, 3).astype(np.int32)


def mass_terms(verts, faces=None):
    """(area (T,), divergence terms (T, 3)) of every triangle in float64, operation for operation as
    oracle.mesh_mass_properties and tri_mass (mesh_regions.h) form them: the numbers both sides add up"""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    t = v.reshape(-1, 3, 3) if faces is None else v[np.asarray(faces, np.int64).reshape(-1, 3)]
    e0, e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], t[:, 2] - t[:, 1]
    u = np.stack([e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1], e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2],
                  e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]], axis=1)
    ln = np.sqrt((u * u).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(ln[:, None] != 0.0, u / ln[:, None], 0.0)
    a = np.sqrt((e1 * e1).sum(1))
    b = np.sqrt((e0 * e0).sum(1))
    c = np.sqrt((e2 * e2).sum(1))
    s = 0.5 * (a + b + c)
    area = np.sqrt(np.abs(s * (s - a) * (s - b) * (s - c)))
    avg = (t[:, 0] + t[:, 1] + t[:, 2]) / 3.0
    return area, area[:, None] * u * avg
