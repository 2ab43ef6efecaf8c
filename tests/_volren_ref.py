"""A float64 numpy restatement of the volume-rendering contract of DESIGN.md section 7d (what csrc/k_volren.hip computes),
vectorised over rays.  Test infrastructure only: the product never imports it.

    prepare(img, shift, kernels)          the uint16 field: shift, then each 5x5 pass in row-major tap order (bit for bit)
    cells(field)                          per 8^3 macro cell (min, max) with a one-voxel apron
    render(field, spacing, setup)         (H, W, 4) float64 RGBA for a volume.render_setup(...) dict
    rays / tri / gradient / headlight     the pieces of render that tests/_maskren_ref.py shares; `ft` np.float32 runs
                                          the interpolation in the kernels' number format
"""
import numpy as np

OPAQUE = 1.0 - 2.0 ** -12
CELL = 8


def prepare(img, shift, kernels):
    v = (img.astype(np.int64) + int(shift)).astype(np.uint16)
    nz, ny, nx = v.shape
    for w in kernels:
        src = v.astype(np.float64)
        acc = np.zeros(v.shape, np.float64)
        for ky in range(5):
            for kx in range(5):
                dy, dx = ky - 2, kx - 2
                term = np.zeros(v.shape, np.float64)  # an out-of-volume tap adds +0.0 to a non-negative sum: skipped
                ys, yd = slice(max(dy, 0), ny + min(dy, 0)), slice(max(-dy, 0), ny + min(-dy, 0))
                xs, xd = slice(max(dx, 0), nx + min(dx, 0)), slice(max(-dx, 0), nx + min(-dx, 0))
                term[:, yd, xd] = w[ky * 5 + kx] * src[:, ys, xs]
                acc = acc + term
        v = acc.astype(np.uint16)  # non-negative: truncation toward zero
    return v


def cells(field):
    nz, ny, nx = field.shape
    cz, cy, cx = [-(-n // CELL) for n in field.shape]
    out = np.zeros((cz, cy, cx, 2), np.uint16)
    for k in range(cz):
        for j in range(cy):
            for i in range(cx):
                blk = field[max(k * CELL - 1, 0):min(k * CELL + CELL, nz - 1) + 1,
                            max(j * CELL - 1, 0):min(j * CELL + CELL, ny - 1) + 1,
                            max(i * CELL - 1, 0):min(i * CELL + CELL, nx - 1) + 1]
                out[k, j, i] = blk.min(), blk.max()
    return out


def tri(v, x, y, z, ft=np.float64):
    nz, ny, nx = v.shape
    x0 = np.minimum(np.floor(x).astype(np.int64), max(nx - 2, 0))
    y0 = np.minimum(np.floor(y).astype(np.int64), max(ny - 2, 0))
    z0 = np.minimum(np.floor(z).astype(np.int64), max(nz - 2, 0))
    fx, fy, fz = x - x0.astype(ft), y - y0.astype(ft), z - z0.astype(ft)
    x1, y1, z1 = np.minimum(x0 + 1, nx - 1), np.minimum(y0 + 1, ny - 1), np.minimum(z0 + 1, nz - 1)

    def f(k, j, i):
        return v[k, j, i].astype(ft)

    def lerp(a, b, t):
        return a + t * (b - a)

    c00 = lerp(f(z0, y0, x0), f(z0, y0, x1), fx)
    c01 = lerp(f(z0, y1, x0), f(z0, y1, x1), fx)
    c10 = lerp(f(z1, y0, x0), f(z1, y0, x1), fx)
    c11 = lerp(f(z1, y1, x0), f(z1, y1, x1), fx)
    return lerp(lerp(c00, c01, fy), lerp(c10, c11, fy), fz)


def gradient(v, x, y, z, hi, ft=np.float64):
    """central differences of the field per two index units, in world axes (world y = -index y)"""
    one = ft(1)
    gx = tri(v, np.minimum(x + one, hi[0]), y, z, ft) - tri(v, np.maximum(x - one, 0), y, z, ft)
    gy = tri(v, x, np.maximum(y - one, 0), z, ft) - tri(v, x, np.minimum(y + one, hi[1]), z, ft)
    gz = tri(v, x, y, np.minimum(z + one, hi[2]), ft) - tri(v, x, y, np.maximum(z - one, 0), ft)
    return gx, gy, gz


def headlight(v, x, y, z, hi, spacing, setup, c, ft=np.float64):
    """the colours `c` (n, 3) at (x, y, z) under the headlight: ambient, diffuse and specular terms of |N . dir| with N
    along the world gradient, in float64 from the gradient's differences on"""
    d = np.asarray(setup["dir"], np.float64)
    gx, gy, gz = [g.astype(np.float64) / (2 * float(s)) for g, s in zip(gradient(v, x, y, z, hi, ft), spacing)]
    gn = np.sqrt(gx * gx + gy * gy + gz * gz)
    ndl = np.where(gn > 0, np.abs(gx * d[0] + gy * d[1] + gz * d[2]) / np.where(gn > 0, gn, 1.0), 0.0)
    diff = setup["ambient"] + setup["diffuse"] * ndl
    spec = np.where(ndl > 0, setup["specular"] * np.power(ndl, setup["specular_power"]), 0.0)
    return np.clip(c * diff[:, None] + spec[:, None], 0.0, 1.0)


def _classify(setup, s, table):
    n = len(setup["alpha"])
    i0 = np.minimum(np.floor(s).astype(np.int64), n - 2)
    f = (s - i0)[:, None]
    return table[i0] + f * (table[i0 + 1] - table[i0])


def rays(shape, spacing, setup, pixels=None):
    """(A, B, hi, tin, kmax): the rays of volren_ray.h in float64 for the field `shape`, of every pixel or of `pixels`
    (rows, cols): index position A + t B at world distance t, the last index per axis, the first sample's distance and
    the last sample's number (-1: the ray misses the box or the clip plane's kept side)"""
    nz, ny, nx = shape
    sx, sy, sz = [float(s) for s in spacing]
    w, h = setup["viewport"]
    if pixels is None:
        py, px = np.mgrid[0:h, 0:w]
    else:
        py, px = np.asarray(pixels[0]), np.asarray(pixels[1])
    px, py = px.ravel().astype(np.float64), py.ravel().astype(np.float64)
    P0 = setup["origin"][None, :] + px[:, None] * setup["du"][None, :] + py[:, None] * setup["dv"][None, :]
    d = np.asarray(setup["dir"], np.float64)
    A = np.stack([P0[:, 0] / sx, -P0[:, 1] / sy, P0[:, 2] / sz], 1)
    B = np.array([d[0] / sx, -d[1] / sy, d[2] / sz])
    hi = np.array([nx - 1, ny - 1, nz - 1], np.float64)
    tin = np.full(len(px), -1e300)
    tout = np.full(len(px), 1e300)
    hit = np.ones(len(px), bool)
    for a in range(3):
        if B[a] != 0.0:
            t0, t1 = (0.0 - A[:, a]) / B[a], (hi[a] - A[:, a]) / B[a]
            tin = np.maximum(tin, np.minimum(t0, t1))
            tout = np.minimum(tout, np.maximum(t0, t1))
        else:
            hit &= (A[:, a] >= 0) & (A[:, a] <= hi[a])
    if setup["clip"] is not None:
        cn, co = setup["clip"]
        nd = float(cn @ d)
        c0 = (P0 - co[None, :]) @ cn
        if nd > 0:
            tin = np.maximum(tin, -c0 / nd)
        elif nd < 0:
            tout = np.minimum(tout, -c0 / nd)
        else:
            hit &= c0 >= 0
    hit &= tin <= tout
    kmax = np.where(hit, np.floor((tout - tin) / np.where(hit, setup["dt"], 1.0)), -1).astype(np.int64)
    return A, B, hi, tin, kmax


def render(field, spacing, setup, pixels=None):
    """`pixels`: optional (rows, cols) index arrays; then the result is (len, 4) for those pixels only"""
    w, h = setup["viewport"]
    A, B, hi, tin, kmax = rays(field.shape, spacing, setup, pixels)
    n = len(tin)
    shape_out = (h, w, 4) if pixels is None else (n, 4)
    dt = setup["dt"]
    bg = np.asarray(setup["background"], np.float64)
    out = np.zeros((n, 4))
    out[:, :3] = bg
    table = np.concatenate([setup["rgba"][:, :3], setup["alpha"][:, None]], 1)
    if setup["mip"]:
        vmax = np.full(n, -1.0)
        for k in range(int(kmax.max(initial=-1)) + 1):
            act = np.nonzero(kmax >= k)[0]
            pos = A[act] + (tin[act] + k * dt)[:, None] * B[None, :]
            pos = np.clip(pos, 0.0, hi[None, :])
            s = tri(field, pos[:, 0], pos[:, 1], pos[:, 2])
            vmax[act] = np.maximum(vmax[act], s)
        got = np.nonzero(vmax >= 0)[0]
        e = _classify(setup, vmax[got], table)
        a = e[:, 3:4]
        out[got, :3] = a * e[:, :3] + (1 - a) * bg[None, :]
        out[got, 3] = a[:, 0]
        return out.reshape(shape_out)
    acc = np.zeros((n, 3))
    alpha = np.zeros(n)
    live = kmax >= 0
    for k in range(int(kmax.max(initial=-1)) + 1):
        act = np.nonzero(live & (kmax >= k))[0]
        if len(act) == 0:
            break
        pos = A[act] + (tin[act] + k * dt)[:, None] * B[None, :]
        pos = np.clip(pos, 0.0, hi[None, :])
        x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
        s = tri(field, x, y, z)
        e = _classify(setup, s, setup["rgba"])
        a = e[:, 3]
        m = a > 0
        act, e, a, x, y, z = act[m], e[m], a[m], x[m], y[m], z[m]
        c = e[:, :3]
        if setup["shade"] and len(act):
            c = headlight(field, x, y, z, hi, spacing, setup, c)
        wgt = (1 - alpha[act]) * a
        acc[act] += wgt[:, None] * c
        alpha[act] += wgt
        live[act[alpha[act] >= OPAQUE]] = False
    out[:, :3] = acc + (1 - alpha)[:, None] * bg[None, :]
    out[:, 3] = alpha
    return out.reshape(shape_out)


def fixture():
    """(presets by name, colour lists by name, the npz) from tests/golden/ref_volume.npz"""
    import json
    import os

    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_volume.npz"))
    presets = json.loads(str(d["presets_json"]))
    cluts = {k[5:]: d[k] for k in d.files if k.startswith("clut_")}
    return presets, cluts, d


def synth_volume(shape, seed=0, shell=3):
    """A CT-like int16 volume whose outer `shell` voxels sit at -1024 (transparent in every preset, smoothing included);
    `shell` 0 leaves the faces as generated"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    f = np.full(shape, -1000.0)
    for _ in range(5):
        c = rng.uniform(0.3, 0.7, 3) * np.array(shape)
        s = rng.uniform(0.12, 0.25) * min(shape)
        amp = rng.uniform(600, 2600)
        f += amp * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * s * s))
    r = np.sqrt(((z - nz / 2) / (nz / 2)) ** 2 + ((y - ny / 2) / (ny / 2)) ** 2 + ((x - nx / 2) / (nx / 2)) ** 2)
    f += 1100.0 * ((r > 0.55) & (r < 0.7))  # a skin-like shell
    f += rng.normal(0, 20, shape)
    img = np.clip(f, -1024, 3071).astype(np.int16)
    if shell > 0:  # img[-0:] would be the whole array
        img[:shell], img[-shell:], img[:, :shell], img[:, -shell:], img[:, :, :shell], img[:, :, -shell:] = (-1024,) * 6
    img[nz // 2, ny // 2, nx // 2] = 3071  # the range's top
    img[shell, shell, shell] = -1024
    return img


def cropped_ct(shape, seed=0):
    """An int16 CT cut through the patient, with material on the box's faces, for any shape down to one voxel per axis
    (voxel centres at (i + 0.5) / n of each axis): a body along z (skin, fat, soft tissue, lungs, two bones, a contrast
    vessel, noise) that runs through the z = 0 and z = nz - 1 slices, and (ny >= 2) a dense table slab in the last rows
    that touches the y = ny - 1 face and both x faces.  Values -1024 .. 3071, both present."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in shape], indexing="ij")
    f = np.full(shape, -1000.0)
    r = np.hypot((x - 0.5) / 0.44, (y - 0.42) / 0.36)
    f[r < 1.0] = 40.0                                         # soft tissue
    f[(r >= 0.80) & (r < 0.92)] = -90.0                       # fat
    f[(r >= 0.92) & (r < 1.0)] = 70.0                         # skin
    for cx in (0.3, 0.7):
        f[np.hypot((x - cx) / 0.13, (y - 0.34) / 0.12) < 1.0] = -550.0  # lungs (partial volume)
    for cx, cy, rad in ((0.32, 0.5, 0.1), (0.7, 0.52, 0.08)):  # bones drifting with z: cortex, marrow
        d = np.hypot(x - cx - 0.06 * np.sin(5.0 * z), y - cy) / rad
        f[d < 1.0] = 1500.0 + 500.0 * z[d < 1.0]
        f[d < 0.55] = 280.0
    f[np.hypot(x - 0.45 - 0.1 * z, y - 0.3) < 0.05] = 330.0  # an oblique contrast vessel
    f += rng.normal(0.0, 25.0, shape)
    if ny >= 2:
        t = ny - max(1, ny // 8)
        f[:, t:, :] = 1400.0 + 300.0 * z[:, t:, :]  # the table
    img = np.clip(f, -1024, 3071).astype(np.int16)
    img.reshape(-1)[0], img.reshape(-1)[-1] = -1024, 3071  # the range's ends
    return img
