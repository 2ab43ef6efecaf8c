"""A float64 numpy restatement of the 3-D scene's rules S1 - S3 (what csrc/k_scene3d.hip computes), vectorised over
rays and built ON the restatements of its parts: tests/_volren_ref.py (rays, tri, _classify, headlight), tests/_maskren_ref.py
(the padded matrix) and tests/_surface_view_ref.py (raster_keys, intensity, the depth order).  Test infrastructure only.

    plane_hit / texel / frag_sample / frag_order   S2 - S3 piece by piece, in the number formats the rules name (float64 hits
                                                   and K_f, float32 depth and texture): csrc/scene3d_math.h must equal them
                                                   bit for bit (tests/test_scene3d_host.py)
    fragments(...)                                 per ray the <= 11 sort keys, colours c I and alphas
    render(...)                                    the picture (H, W, 4) float64 with the per-ray counts: samples taken, K_f per
                                                   layer, the fragment order, rays that hit the box
    ray_t / surface_t                              S1's two depths of one world point

A plane is a dict: orientation ("AXIAL" / "CORONAL" / "SAGITAL"), n, picture (h, w, 3) uint8, opacity."""
import numpy as np

import _surface_view_ref as SR
import _volren_ref as R
from _volren_ref import _classify, headlight, rays  # noqa: F401  (the scene composites with the ray casters' own pieces)
from _surface_view_ref import intensity, raster_keys  # noqa: F401

OPAQUE = R.OPAQUE
EMPTY = SR.EMPTY
MAX_LAYERS, MAX_PLANES = 8, 3
MAX_FRAGS = MAX_LAYERS + MAX_PLANES
ORIENTATIONS = {"AXIAL": 0, "CORONAL": 1, "SAGITAL": 2}
NONE, IMAGE, MASK = 0, 1, 2
HI32 = np.uint64(0xFFFFFFFF00000000)


def plane(orientation, n, picture, opacity=1.0):
    return {"orientation": orientation, "n": int(n), "picture": np.ascontiguousarray(picture, np.uint8), "opacity": float(opacity)}


def pixel_origins(setup, pixels=None):
    """P0 = origin + i du + j dv of every pixel (row-major) or of `pixels` (rows, cols)"""
    w, h = setup["viewport"]
    if pixels is None:
        py, px = np.mgrid[0:h, 0:w]
    else:
        py, px = np.asarray(pixels[0]), np.asarray(pixels[1])
    px, py = px.ravel().astype(np.float64), py.ravel().astype(np.float64)
    return setup["origin"][None, :] + px[:, None] * setup["du"][None, :] + py[:, None] * setup["dv"][None, :]


def plane_hit(P0, d, spacing, orientation, n, h, w, off=0):
    """S2: (hit, t float32, u float32, v float32) of the rays P0 + t d on the plane; `off` 1 on the padded mask matrix"""
    o = ORIENTATIONS[orientation] if isinstance(orientation, str) else int(orientation)
    a = {0: 2, 1: 1, 2: 0}[o]
    s = [float(x) for x in spacing]
    d = [float(x) for x in d]
    cnt = len(P0)
    if d[a] == 0.0:
        return np.zeros(cnt, bool), np.zeros(cnt, np.float32), np.zeros(cnt, np.float32), np.zeros(cnt, np.float32)
    nn = float(int(n) + int(off))
    c = -(nn * s[1]) if a == 1 else nn * s[a]
    with np.errstate(all="ignore"):
        tp = (c - P0[:, a]) / d[a]
        qx, qy, qz = P0[:, 0] + tp * d[0], P0[:, 1] + tp * d[1], P0[:, 2] + tp * d[2]
        ix, iy, iz = qx / s[0] - float(off), -qy / s[1] - float(off), qz / s[2] - float(off)
        du = iy if a == 0 else ix
        dv = iy if a == 2 else iz
        hit = (0.0 <= du) & (du <= float(w - 1)) & (0.0 <= dv) & (dv <= float(h - 1))
        return hit, tp.astype(np.float32), np.where(hit, du, 0.0).astype(np.float32), np.where(hit, dv, 0.0).astype(np.float32)


def texel(picture, u, v):
    """S2: the RGB8 picture at column position u, row position v: bilinear in float32, columns first, then / 255"""
    pic = np.asarray(picture, np.uint8)
    h, w = pic.shape[:2]
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    i0 = np.minimum(u.astype(np.int64), max(w - 2, 0))
    j0 = np.minimum(v.astype(np.int64), max(h - 2, 0))
    i1, j1 = np.minimum(i0 + 1, w - 1), np.minimum(j0 + 1, h - 1)
    fu, fv = (u - i0.astype(np.float32))[:, None], (v - j0.astype(np.float32))[:, None]
    f = pic.astype(np.float32)

    def lerp(a, b, t):
        return a + t * (b - a)

    top = lerp(f[j0, i0], f[j0, i1], fu)
    bot = lerp(f[j1, i0], f[j1, i1], fu)
    out = lerp(top, bot, fv) / np.float32(255.0)
    assert out.dtype == np.float32
    return out


def frag_sample(t32, tin, dt, kmax):
    """S3: K_f = clamp(ceil((double(t) - tin) / dt), 0, kmax + 1); a ray without samples (kmax -1) gives 0"""
    t = np.asarray(t32, np.float32).astype(np.float64)
    kmax = np.asarray(kmax, np.int64)
    with np.errstate(all="ignore"):
        k = np.ceil((t - np.asarray(tin, np.float64)) / float(dt))
    k = np.where(k > 0.0, k, 0.0)  # (a number that is none included)
    return np.minimum(k, (kmax + 1).astype(np.float64)).astype(np.int64)


def frag_key(t32, layer):
    bits = np.asarray(t32, np.float32).view(np.uint32)
    return (SR.ord_of(bits).astype(np.uint64) << np.uint64(32)) | np.uint64(layer)


def key_depth(key):
    return SR.bits_of((np.asarray(key, np.uint64) >> np.uint64(32)).astype(np.uint32)).view(np.float32)


def frag_order(sk):
    """S2: the layers of a ray's fragments near to far by (ord depth, layer); -1 past the last.  sk: (MAX_FRAGS, n)"""
    order = np.argsort(sk, axis=0, kind="stable")
    return np.where(np.take_along_axis(sk, order, 0) != EMPTY, order, -1)


def fragments(setup, spacing, layers=(), cam=None, mode=SR.GOURAUD, planes=(), off=0, keys=None, pixels=None):
    """(sk, colour, alpha): (MAX_FRAGS, n) uint64 sort keys (all ones: no fragment), (MAX_FRAGS, n, 3) float64 c I and
    (MAX_FRAGS,) float64 alphas; surfaces are layers 0 .. 7 in scene order, planes 8, 9, 10"""
    if len(layers) > MAX_LAYERS:
        raise ValueError("at most %d surfaces" % MAX_LAYERS)
    if len(planes) > MAX_PLANES or len({p["orientation"] for p in planes}) != len(planes):
        raise ValueError("at most %d planes, one per orientation" % MAX_PLANES)
    P0 = pixel_origins(setup, pixels)
    n = len(P0)
    sk = np.full((MAX_FRAGS, n), EMPTY, np.uint64)
    col = np.zeros((MAX_FRAGS, n, 3))
    alpha = np.zeros(MAX_FRAGS)
    if layers:
        if keys is None:
            keys = [SR.raster_keys(L["verts"], L["faces"], cam) for L in layers]
        sel = slice(None) if pixels is None else (np.asarray(pixels[0]).ravel(), np.asarray(pixels[1]).ravel())
        for k, (L, K) in enumerate(zip(layers, keys)):
            I = SR.intensity(L, K, cam, mode)[sel].ravel()
            Kf = K[sel].ravel()
            sk[k] = np.where(Kf != EMPTY, (Kf & HI32) | np.uint64(k), EMPTY)
            rgb = np.asarray(L["colour"], np.float32).astype(np.float64)
            col[k] = rgb[None, :] * I[:, None]
            alpha[k] = float(np.float32(L["opacity"]))
    for p in planes:
        o = ORIENTATIONS[p["orientation"]]
        h, w = p["picture"].shape[:2]
        hit, t, u, v = plane_hit(P0, setup["dir"], spacing, o, p["n"], h, w, off)
        sk[MAX_LAYERS + o] = np.where(hit, frag_key(t, MAX_LAYERS + o), EMPTY)
        col[MAX_LAYERS + o][hit] = texel(p["picture"], u[hit], v[hit]).astype(np.float64)
        alpha[MAX_LAYERS + o] = float(np.float32(p["opacity"]))
    return sk, col, alpha


def render(field, spacing, setup, layers=(), cam=None, mode=SR.GOURAUD, planes=(), kind=IMAGE, keys=None, pixels=None):
    """S1 - S3.  `field`: the prepared uint16 field (IMAGE), the padded uint8 matrix (MASK) or None (NONE); `setup`:
    volume.render_setup / volume_mask.render_setup / scene3d's no-field numbers.  Returns a dict: image (H, W, 4) float64 (or
    (len, 4) with `pixels`), taken (samples classified per ray), kf (MAX_FRAGS, n) K_f per layer (-1: no fragment), order
    (MAX_FRAGS, n) layers near to far, hit (rays that meet the box)."""
    assert not setup["mip"], "the scene composites"
    w, h = setup["viewport"]
    sk, col, alpha = fragments(setup, spacing, layers, cam, mode, planes, 1 if kind == MASK else 0, keys, pixels)
    n = sk.shape[1]
    dt = float(setup["dt"])
    if kind == NONE:
        tin, kmax = np.zeros(n), np.full(n, -1, np.int64)
        A = B = hi = None
    else:
        A, B, hi, tin, kmax = R.rays(field.shape, spacing, setup, pixels)
    has = sk != EMPTY
    kf = np.where(has, frag_sample(key_depth(sk), np.where(kmax >= 0, tin, 0.0)[None, :], dt, kmax[None, :]), -1)
    order = frag_order(sk)
    bg = np.asarray(setup["background"], np.float64)
    acc = np.zeros((n, 3))
    alp = np.zeros(n)
    live = np.ones(n, bool)
    taken = np.zeros(n, np.int64)
    # per rank the layer, its K_f, colour and alpha
    rank_layer = order
    ar = np.arange(n)
    for k in range(int(kmax.max(initial=-1)) + 2):
        for r in range(MAX_FRAGS):  # the fragments that go before sample k, near to far
            lay = rank_layer[r]
            idx = np.nonzero(live & (lay >= 0) & (kf[np.maximum(lay, 0), ar] == k))[0]
            if not len(idx):
                continue
            ly = lay[idx]
            wgt = (1.0 - alp[idx]) * alpha[ly]
            acc[idx] += wgt[:, None] * col[ly, idx]
            alp[idx] += wgt
            live[idx[alp[idx] >= OPAQUE]] = False
        act = np.nonzero(live & (kmax >= k))[0]
        if not len(act):
            continue
        pos = A[act] + (tin[act] + k * dt)[:, None] * B[None, :]
        pos = np.clip(pos, 0.0, hi[None, :])
        x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
        s = R.tri(field, x, y, z)
        taken[act] += 1
        e = R._classify(setup, s, setup["rgba"])
        a = e[:, 3]
        m = a > 0
        act, e, a, x, y, z = act[m], e[m], a[m], x[m], y[m], z[m]
        c = e[:, :3]
        if setup["shade"] and len(act):
            c = R.headlight(field, x, y, z, hi, spacing, setup, c)
        wgt = (1.0 - alp[act]) * a
        acc[act] += wgt[:, None] * c
        alp[act] += wgt
        live[act[alp[act] >= OPAQUE]] = False
    out = np.concatenate([acc + (1.0 - alp)[:, None] * bg[None, :], alp[:, None]], 1)
    return {"image": out.reshape((h, w, 4) if pixels is None else (n, 4)), "taken": taken, "kf": kf, "order": order,
            "hit": kmax >= 0, "early": ~live}


def to_rgba8(img):
    """write_pixel's rule on the float32 picture: floor(255 v + 0.5) in float32, clamped to 0 .. 255"""
    v = np.asarray(img, np.float32)
    return np.clip(np.floor(np.float32(255.0) * v + np.float32(0.5)), np.float32(0.0), np.float32(255.0)).astype(np.uint8)


# ---- S1: one depth axis -----------------------------------------------------------------------------------------------------
def surface_t(cam, point):
    """R3's depth of a world point: (v - focal) . dir in R1's order, rounded to float32"""
    f, d = cam["focal"], cam["dir"]
    dx, dy, dz = float(point[0]) - float(f[0]), float(point[1]) - float(f[1]), float(point[2]) - float(f[2])
    return np.float32((dx * float(d[0]) + dy * float(d[1])) + dz * float(d[2]))


def ray_t(setup, point):
    """the distance along its ray of a world point from the pixel plane of `setup` (whatever pixel the point falls on):
    (point - origin) . dir; du and dv are orthogonal to dir"""
    d = np.asarray(setup["dir"], np.float64)
    return float((np.asarray(point, np.float64) - setup["origin"]) @ d)
