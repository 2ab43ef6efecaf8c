"""numpy float64 restatement of the surface view's rules R1 - R5, independent of the product's Python and C++:
parallel projection, front-face coverage, the order-free (depth, triangle) key, flat / Gouraud / Phong intensity under one
headlight, and the sorted composition of up to eight surfaces.

Every expression is written in the order the rules state, so the GPU path must agree bit for bit.  The rasteriser runs
serially over the triangles and is vectorised over each triangle's pixel box; the resolve is vectorised over the pixels.

A camera is a dict with focal, right, up, dir (3 floats each), parallel_scale and viewport (W, H).
A layer is a dict with verts (n, 3) float32, faces (m, 3) int32, normals (n, 3) float32 or None, colour (3) and transparency."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
FLAT, GOURAUD, PHONG = 0, 1, 2
MAX_LAYERS = 8


def _dot(dx, dy, dz, a):
    return (dx * float(a[0]) + dy * float(a[1])) + dz * float(a[2])


def project(verts, cam):
    """R1: (X, Y, t, finite) of every point, float64"""
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    v = v32.astype(np.float64)
    W, H = cam["viewport"]
    px = 2.0 * float(cam["parallel_scale"]) / float(H)
    f = cam["focal"]
    with np.errstate(all="ignore"):
        dx, dy, dz = v[:, 0] - float(f[0]), v[:, 1] - float(f[1]), v[:, 2] - float(f[2])
        X = _dot(dx, dy, dz, cam["right"]) / px + 0.5 * float(W)
        Y = 0.5 * float(H) - _dot(dx, dy, dz, cam["up"]) / px
        t = _dot(dx, dy, dz, cam["dir"])
    return X, Y, t, np.isfinite(v32).all(axis=1)


def _edge(ax, ay, ia, bx, by, ib, qx, qy):
    """edge function of a -> b at q, evaluated from the end point with the smaller vertex id"""
    swap = ia > ib
    px, py = np.where(swap, bx, ax), np.where(swap, by, ay)
    ex, ey = np.where(swap, ax, bx), np.where(swap, ay, by)
    with np.errstate(all="ignore"):
        e = (ex - px) * (qy - py) - (ey - py) * (qx - px)
    return np.where(swap, -e, e)


def _span(lo, hi, n):
    p0 = np.ceil(np.minimum(np.maximum(lo - 0.5, 0.0), float(n))).astype(np.int64)
    p1 = np.floor(np.minimum(np.maximum(hi - 0.5, -1.0), float(n - 1))).astype(np.int64)
    return p0, p1


def ord_of(bits):
    """float32 bits -> unsigned order (R3)"""
    bits = np.asarray(bits, np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)


def bits_of(o):
    o = np.asarray(o, np.uint32)
    return np.where(o & np.uint32(0x80000000), o ^ np.uint32(0x80000000), ~o).astype(np.uint32)


def pixel_boxes(X, Y, fin, faces, size):
    """per triangle: drawable?, x0, x1, y0, y1 (inclusive, clamped) and the signed area (R2)"""
    W, H = size
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    ok = fin[a] & fin[b] & fin[c] & (a != b) & (b != c) & (a != c)
    area = _edge(X[a], Y[a], a, X[b], Y[b], b, X[c], Y[c])
    with np.errstate(invalid="ignore"):
        ok &= area < 0.0  # front faces only; zero and not-a-number draw nothing
    sx, sy = np.where(ok[:, None], X[f], 0.0), np.where(ok[:, None], Y[f], 0.0)
    x0, x1 = _span(sx.min(1), sx.max(1), W)
    y0, y1 = _span(sy.min(1), sy.max(1), H)
    ok &= (x1 >= x0) & (y1 >= y0)
    return ok, x0, x1, y0, y1, area


def raster_keys(verts, faces, cam):
    """R2 + R3: uint64 keys (H, W) of one surface; all ones where nothing is drawn"""
    W, H = cam["viewport"]
    keys = np.full((H, W), EMPTY, np.uint64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if not len(f):
        return keys
    X, Y, t, fin = project(verts, cam)
    ok, x0, x1, y0, y1, area = pixel_boxes(X, Y, fin, f, (W, H))
    for tri in np.nonzero(ok)[0]:
        a, b, c = f[tri]
        j, i = np.mgrid[y0[tri]:y1[tri] + 1, x0[tri]:x1[tri] + 1]
        qx, qy = i + 0.5, j + 0.5
        e_ab = _edge(X[a], Y[a], a, X[b], Y[b], b, qx, qy)
        e_bc = _edge(X[b], Y[b], b, X[c], Y[c], c, qx, qy)
        e_ca = _edge(X[c], Y[c], c, X[a], Y[a], a, qx, qy)
        inside = (e_ab <= 0.0) & (e_bc <= 0.0) & (e_ca <= 0.0)
        if not inside.any():
            continue
        with np.errstate(all="ignore"):
            d = (((e_bc * t[a] + e_ca * t[b]) + e_ab * t[c]) / area[tri]).astype(np.float32)
        key = (ord_of(d.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | np.uint64(tri)
        box = keys[y0[tri]:y1[tri] + 1, x0[tri]:x1[tri] + 1]
        box[inside] = np.minimum(box[inside], key[inside])
    return keys


def _headlight(nx, ny, nz, d):
    s = -((nx * float(d[0]) + ny * float(d[1])) + nz * float(d[2]))
    return np.where(s > 0.0, s, 0.0)


def _headlight_unit(nx, ny, nz, d):
    ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
    good = ln > 0.0
    safe = np.where(good, ln, 1.0)
    return np.where(good, _headlight(nx / safe, ny / safe, nz / safe, d), 0.0)


def intensity(layer, keys, cam, mode):
    """R4: float64 intensity (H, W) of the layer's winning triangles; 0 where the layer has no fragment"""
    W, H = cam["viewport"]
    out = np.zeros((H, W), np.float64)
    jj, ii = np.nonzero(keys != EMPTY)
    if not len(jj):
        return out
    tri = (keys[jj, ii] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    f = np.asarray(layer["faces"], np.int64).reshape(-1, 3)[tri]
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    v = np.asarray(layer["verts"], np.float32).reshape(-1, 3).astype(np.float64)
    normals = layer.get("normals")
    if mode == FLAT or normals is None:
        u, w = v[b] - v[a], v[c] - v[a]
        out[jj, ii] = _headlight_unit(u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                                      u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0], cam["dir"])
        return out
    X, Y, _, _ = project(layer["verts"], cam)
    qx, qy = ii + 0.5, jj + 0.5
    area = _edge(X[a], Y[a], a, X[b], Y[b], b, X[c], Y[c])
    la = _edge(X[b], Y[b], b, X[c], Y[c], c, qx, qy) / area
    lb = _edge(X[c], Y[c], c, X[a], Y[a], a, qx, qy) / area
    lc = _edge(X[a], Y[a], a, X[b], Y[b], b, qx, qy) / area
    n = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    na, nb, nc = n[a], n[b], n[c]
    if mode == GOURAUD:
        ia, ib, ic = (_headlight(m[:, 0], m[:, 1], m[:, 2], cam["dir"]) for m in (na, nb, nc))
        out[jj, ii] = (la * ia + lb * ib) + lc * ic
        return out
    s = [(la * na[:, q] + lb * nb[:, q]) + lc * nc[:, q] for q in range(3)]
    out[jj, ii] = _headlight_unit(s[0], s[1], s[2], cam["dir"])
    return out


def to_rgba8(img):
    return np.clip(np.floor(255.0 * np.asarray(img, np.float32).astype(np.float64) + 0.5), 0, 255).astype(np.uint8)


def render(layers, cam, mode=GOURAUD, background=(0.0, 0.0, 0.0), keys=None):
    """R1 - R5: dict with keys (one (H, W) uint64 per layer), rgba float32 (H, W, 4), rgba8, ids int32 (H, W, 2), depth float32"""
    if len(layers) > MAX_LAYERS:
        raise TypeError("at most %d surfaces" % MAX_LAYERS)
    W, H = cam["viewport"]
    if keys is None:
        keys = [raster_keys(L["verts"], L["faces"], cam) for L in layers]
    n = len(layers)
    bg = np.asarray(background, np.float32).astype(np.float64)
    C = np.broadcast_to(bg, (H, W, 3)).copy()
    A = np.zeros((H, W), np.float64)
    ids = np.full((H, W, 2), -1, np.int32)
    depth = np.full((H, W), np.inf, np.float32)
    if n:
        alpha32 = np.array([L["opacity"] for L in layers], np.float32)
        alpha = alpha32.astype(np.float64)
        rgb = np.array([np.asarray(L["colour"], np.float32) for L in layers], np.float32).astype(np.float64)
        K = np.stack(keys)                                                           # (n, H, W)
        has = K != EMPTY
        layer_no = np.arange(n, dtype=np.uint64)[:, None, None]
        sk = np.where(has, (K & np.uint64(0xFFFFFFFF00000000)) | layer_no, EMPTY)     # (ord depth, layer index)
        opaque = (alpha32 == np.float32(1.0))[:, None, None]
        cut = np.where(has & opaque, sk, EMPTY).min(axis=0)
        live = has & (sk <= cut)
        I = np.stack([intensity(L, k, cam, mode) for L, k in zip(layers, keys)])
        order = np.argsort(sk, axis=0, kind="stable")                                # near ... far, the empty ones last
        for pos in range(n - 1, -1, -1):                                             # far to near
            k = order[pos]
            lv = np.take_along_axis(live, k[None], 0)[0]
            Ik = np.take_along_axis(I, k[None], 0)[0]
            al, col = alpha[k], rgb[k]
            blend = (al[..., None] * col) * Ik[..., None] + (1.0 - al)[..., None] * C
            solid = col * Ik[..., None]
            newC = np.where((alpha32[k] == np.float32(1.0))[..., None], solid, blend)
            newA = np.where(alpha32[k] == np.float32(1.0), 1.0, al + (1.0 - al) * A)
            C = np.where(lv[..., None], newC, C)
            A = np.where(lv, newA, A)
        near = sk.min(axis=0)
        hit = near != EMPTY
        k0 = np.where(hit, near & np.uint64(7), np.uint64(0)).astype(np.int64)
        ids[..., 0] = np.where(hit, k0, -1)
        ids[..., 1] = np.where(hit, (np.take_along_axis(K, k0[None], 0)[0] & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
        depth = np.where(hit, bits_of((near >> np.uint64(32)).astype(np.uint32)).view(np.float32), np.float32(np.inf)).astype(np.float32)
    rgba = np.concatenate([C, A[..., None]], axis=-1).astype(np.float32)
    return {"keys": keys, "rgba": rgba, "rgba8": to_rgba8(rgba), "ids": ids, "depth": depth}


def layer(verts, faces, normals=None, colour=(1.0, 1.0, 1.0), transparency=0.0):
    """opacity is float32(1 - transparency), the number the C ABI carries"""
    return {"verts": np.ascontiguousarray(verts, np.float32).reshape(-1, 3), "faces": np.ascontiguousarray(faces, np.int32).reshape(-1, 3),
            "normals": None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3),
            "colour": tuple(float(x) for x in colour), "transparency": float(transparency),
            "opacity": np.float32(1.0 - float(transparency))}


def pick(result, cam, layers, col, row):
    """what Scene.pick returns: surface, triangle, world position (pixel_rays' centre + t dir), nearest corner's id"""
    s, tri = (int(x) for x in result["ids"][row, col])
    if s < 0:
        return None
    W, H = cam["viewport"]
    px = 2.0 * float(cam["parallel_scale"]) / H
    r, u, d, f = (np.asarray(cam[k], np.float64) for k in ("right", "up", "dir", "focal"))
    origin = f + (r * px) * (0.5 - W / 2.0) + (-u * px) * (0.5 - H / 2.0)
    pos = origin + (r * px) * col + (-u * px) * row + float(result["depth"][row, col]) * d
    corners = layers[s]["faces"][tri]
    dist = ((layers[s]["verts"][corners].astype(np.float64) - pos) ** 2).sum(axis=1)
    return {"surface": s, "triangle": tri, "position": pos, "point_id": int(corners[int(np.argmin(dist))])}
