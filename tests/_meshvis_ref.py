"""numpy float64 restatement of the surface visibility rules, independent of the product's Python: cameras from
the bounds, projection, a depth-only rasteriser (per triangle over its clamped pixel box, edge functions evaluated from the
smaller vertex id, float32 rounding, minimum), vtkSelectVisiblePoints' point test and the any-corner selection.

Every expression is written in the order the rules state, so the GPU path must agree bit for bit.  Triangles are processed in
groups of equal (power of two) box size, vectorised over group x box: the element-wise arithmetic is that of one triangle."""
import math

import numpy as np

POSITIONS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
TOLERANCE = 0.01
ONE_BITS = np.uint32(0x3F800000)


def bounds_of(verts):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    if not len(v):
        return (0.0,) * 6
    lo, hi = v.min(0), v.max(0)
    return (float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1]), float(lo[2]), float(hi[2]))


def views(bounds, positions=POSITIONS, size=(800, 800)):
    W, H = int(size[0]), int(size[1])
    b = [float(x) for x in bounds]
    c = [(b[0] + b[1]) / 2, (b[2] + b[3]) / 2, (b[4] + b[5]) / 2]
    w = [b[1] - b[0], b[3] - b[2], b[5] - b[4]]
    radius = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) * 0.5
    if radius == 0.0:
        radius = 1.0
    half = math.radians(30.0) * 0.5
    dist = radius / math.sin(half)
    up = [0.0, 1.0, 0.0]
    out = []
    for p in positions:
        p = [float(x) for x in p]
        ln = math.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
        n = [p[0] / ln, p[1] / ln, p[2] / ln]
        eye = [c[q] + n[q] * dist for q in range(3)]
        if abs(up[0] * n[0] + up[1] * n[1] + up[2] * n[2]) > 0.999:
            up = [-up[2], up[0], up[1]]
        fwd = [-n[0], -n[1], -n[2]]
        r = _cross(fwd, up)
        ln = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
        right = [r[0] / ln, r[1] / ln, r[2] / ln]
        upv = _cross(right, fwd)
        n0, f0 = math.inf, -math.inf
        for x in (b[0], b[1]):
            for y in (b[2], b[3]):
                for z in (b[4], b[5]):
                    d = ((x - eye[0]) * fwd[0] + (y - eye[1]) * fwd[1]) + (z - eye[2]) * fwd[2]
                    n0, f0 = min(n0, d), max(f0, d)
        near = 0.99 * n0 - 0.5 * (f0 - n0)
        far = 1.01 * f0 + 0.5 * (f0 - near)
        if near >= far:
            near = 0.01 * far
        near = max(near, 0.001 * far)
        out.append({"eye": eye, "right": right, "up": upv, "fwd": fwd, "near": near, "far": far, "tan_half": math.tan(half),
                    "aspect": W / H, "size": (W, H), "view_up": list(up), "dist": dist, "centre": c})
    return out


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def project(verts, view):
    """(xs, ys, zw, in_front) of every point, float64"""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    W, H = view["size"]
    e, r, u, f = view["eye"], view["right"], view["up"], view["fwd"]
    dx, dy, dz = v[:, 0] - e[0], v[:, 1] - e[1], v[:, 2] - e[2]
    xe = (dx * r[0] + dy * r[1]) + dz * r[2]
    ye = (dx * u[0] + dy * u[1]) + dz * u[2]
    ze = (dx * f[0] + dy * f[1]) + dz * f[2]
    front = ze > 0.0
    with np.errstate(all="ignore"):
        xs = (xe / (ze * view["tan_half"] * view["aspect"]) + 1) * 0.5 * W
        ys = (ye / (ze * view["tan_half"]) + 1) * 0.5 * H
        zw = (view["far"] * (ze - view["near"])) / (ze * (view["far"] - view["near"]))
    return xs, ys, zw, front


def _edge(ax, ay, ia, bx, by, ib, qx, qy):
    """edge function of a -> b at q, evaluated from the end point with the smaller vertex id"""
    swap = ia > ib
    px, py = np.where(swap, bx, ax), np.where(swap, by, ay)
    ex, ey = np.where(swap, ax, bx), np.where(swap, ay, by)
    e = (ex - px) * (qy - py) - (ey - py) * (qx - px)
    return np.where(swap, -e, e)


def _span(lo, hi, n):
    p0 = np.ceil(np.minimum(np.maximum(lo - 0.5, 0.0), float(n))).astype(np.int64)
    p1 = np.floor(np.minimum(np.maximum(hi - 0.5, -1.0), float(n - 1))).astype(np.int64)
    return p0, p1


def pixel_boxes(xs, ys, front, faces, size):
    """per triangle: drawable?, x0, x1, y0, y1 (inclusive, clamped) and the signed area"""
    W, H = size
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    ok = front[a] & front[b] & front[c] & (a != b) & (b != c) & (a != c)
    area = _edge(xs[a], ys[a], a, xs[b], ys[b], b, xs[c], ys[c])
    ok &= area != 0.0
    ok &= ~np.isnan(area)
    x0, x1 = _span(np.minimum(np.minimum(xs[a], xs[b]), xs[c]), np.maximum(np.maximum(xs[a], xs[b]), xs[c]), W)
    y0, y1 = _span(np.minimum(np.minimum(ys[a], ys[b]), ys[c]), np.maximum(np.maximum(ys[a], ys[b]), ys[c]), H)
    ok &= (x1 >= x0) & (y1 >= y0)
    return ok, x0, x1, y0, y1, area


def raster_screen(xs, ys, zw, front, faces, size):
    """float32 depth (H, W) from screen-space points"""
    W, H = size
    bits = np.full(W * H, ONE_BITS, np.uint32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if not len(f):
        return bits.view(np.float32).reshape(H, W)
    ok, x0, x1, y0, y1, area = pixel_boxes(xs, ys, front, f, size)
    idx = np.nonzero(ok)[0]
    bw, bh = (x1 - x0 + 1)[idx], (y1 - y0 + 1)[idx]
    steps = np.unique(np.concatenate([[1, 2, 3], (np.array([[4], [5], [6]]) << np.arange(32)).ravel()]))  # 1 2 3 4 5 6 8 10 12 16 ...
    cw, ch = steps[np.searchsorted(steps, bw)], steps[np.searchsorted(steps, bh)]
    for gw, gh in sorted(set(zip(cw.tolist(), ch.tolist()))):
        grp = idx[(cw == gw) & (ch == gh)]
        step = max(1, (1 << 20) // (gw * gh))
        oi, oj = np.meshgrid(np.arange(gw), np.arange(gh))
        oi, oj = oi.reshape(1, -1), oj.reshape(1, -1)
        for s in range(0, len(grp), step):
            t = grp[s:s + step]
            a, b, c = f[t, 0][:, None], f[t, 1][:, None], f[t, 2][:, None]
            i, j = x0[t][:, None] + oi, y0[t][:, None] + oj
            inbox = (i <= x1[t][:, None]) & (j <= y1[t][:, None])
            qx, qy = i + 0.5, j + 0.5
            e_ab = _edge(xs[a], ys[a], a, xs[b], ys[b], b, qx, qy)
            e_bc = _edge(xs[b], ys[b], b, xs[c], ys[c], c, qx, qy)
            e_ca = _edge(xs[c], ys[c], c, xs[a], ys[a], a, qx, qy)
            ar = area[t][:, None]
            inside = np.where(ar > 0.0, (e_ab >= 0.0) & (e_bc >= 0.0) & (e_ca >= 0.0), (e_ab <= 0.0) & (e_bc <= 0.0) & (e_ca <= 0.0))
            z = ((((e_bc * zw[a] + e_ca * zw[b]) + e_ab * zw[c]) / ar).astype(np.float32)).view(np.uint32)
            hit = inbox & inside & (z < ONE_BITS)
            np.minimum.at(bits, (j * W + i)[hit], z[hit])
    return bits.view(np.float32).reshape(H, W)


def depth_buffer(verts, faces, view):
    xs, ys, zw, front = project(verts, view)
    return raster_screen(xs, ys, zw, front, faces, view["size"])


def covered(depth):
    return depth < np.float32(1.0)


def visible_in_view(verts, depth, view):
    W, H = view["size"]
    xs, ys, zw, front = project(verts, view)
    with np.errstate(invalid="ignore"):
        inside = front & (xs >= 0.0) & (xs < W) & (ys >= 0.0) & (ys < H)
    i = np.where(inside, xs, 0.0).astype(np.int64)
    j = np.where(inside, ys, 0.0).astype(np.int64)
    return inside & (zw < depth[j, i].astype(np.float64) + TOLERANCE)


def visible_points(verts, faces, positions=POSITIONS, size=(800, 800), view_list=None):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    flags = np.zeros(len(v), bool)
    if view_list is None:
        view_list = views(bounds_of(v), positions, size)
    for view in view_list:
        flags |= visible_in_view(v, depth_buffer(v, faces, view), view)
    return flags.astype(np.uint8)


def select(verts, faces, flags, invert=False):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    fl = (np.asarray(flags) != 0) != bool(invert)
    keep = fl[f].any(axis=1) if len(f) else np.zeros(0, bool)
    kf = f[keep]
    used = np.zeros(len(v), bool)
    used[kf.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return v[used], remap[kf].astype(np.int32).reshape(-1, 3)


def remove_non_visible_faces(verts, faces, positions=POSITIONS, remove_visible=False, size=(800, 800)):
    return select(verts, faces, visible_points(verts, faces, positions, size), remove_visible)


def has_non_visible_faces(verts, faces, threshold=0.7, positions=POSITIONS, size=(800, 800)):
    n = len(np.asarray(verts).reshape(-1, 3))
    if n == 0:
        return False
    return int(visible_points(verts, faces, positions, size).sum()) / n < threshold
