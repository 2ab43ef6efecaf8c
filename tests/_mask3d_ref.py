"""numpy float64 restatements of mask_cut.rs and brush_mask.rs, and the cases the 3-D mask editor's tests share
(tests/test_mask3d_editor_host.py on the CPU, tests/test_gpu_mask3d_editor.py on the GPU)."""
import numpy as np

VALUES = np.array([0, 1, 127, 128, 254, 255], np.uint8)


def volume(shape, seed, fill=None):
    """a (d, h, w) interior of the values either side of every threshold the rules have (> 127, > 0)"""
    if fill is not None:
        return np.full(shape, fill, np.uint8)
    rng = np.random.default_rng(seed)
    return VALUES[rng.integers(0, len(VALUES), shape)]


def padded(interior, guard=True):
    """the padded matrix of an interior; the flag planes hold guard values no rule produces"""
    d, h, w = interior.shape
    m = np.zeros((d + 1, h + 1, w + 1), np.uint8)
    if guard:
        m[0] = 37
        m[:, 0, :] = 41
        m[:, :, 0] = 43
    m[1:, 1:, 1:] = interior
    return m


def row_dot(a, i, p0, p1, p2):
    return ((a[i, 0] * p0 + a[i, 1] * p1) + a[i, 2] * p2) + a[i, 3] * 1.0


def np_mask_cut(vol, sx, sy, sz, max_depth, filt, m, mv, edit_mode):
    """mask_cut.rs:30-60 on a copy of the (d, h, w) volume: float64, every product and sum rounded on its own"""
    out = vol.copy()
    d, h, w = vol.shape
    mh, mw = filt.shape
    z, y, x = np.meshgrid(np.arange(d, dtype=np.float64), np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    p0, p1, p2 = x * sx, y * sy, z * sz
    m, mv = np.asarray(m, np.float64), np.asarray(mv, np.float64)
    with np.errstate(all="ignore"):
        q3 = row_dot(m, 3, p0, p1, p2)
        q0, q1 = row_dot(m, 0, p0, p1, p2) / q3, row_dot(m, 1, p0, p1, p2) / q3
        c3 = row_dot(mv, 3, p0, p1, p2)
        c0, c1, c2 = row_dot(mv, 0, p0, p1, p2) / c3, row_dot(mv, 1, p0, p1, p2) / c3, row_dot(mv, 2, p0, p1, p2) / c3
        dist = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
        px = (q0 / 2.0 + 0.5) * float(mw - 1)
        py = (q1 / 2.0 + 0.5) * float(mh - 1)
        live = (vol > 127) & (q3 > 0.0) & (dist <= max_depth)
        on = (px >= 0.0) & (px < float(mw)) & (py >= 0.0) & (py < float(mh))
    iy = np.where(on, py, 0.0).astype(np.int64)
    ix = np.where(on, px, 0.0).astype(np.int64)
    hit = np.zeros(vol.shape, bool)
    if mh and mw:
        hit = np.asarray(filt, bool)[np.clip(iy, 0, mh - 1), np.clip(ix, 0, mw - 1)]
    zero = live & ((on & hit) | (~on & (edit_mode == 0)))
    out[zero] = 0
    return out


def np_brush(vol, orig, spacing, center, radius, edit_mode):
    """brush_mask.rs:24-69 on a copy"""
    out = vol.copy()
    d, h, w = vol.shape
    sx, sy, sz = spacing
    cx, cy, cz = center

    def lo(c, s):
        return int(max(np.floor((c - radius) / s), 0.0))

    def hi(c, s, n):
        return int(min(max(np.ceil((c + radius) / s), 0.0), float(n - 1)))

    x0, x1, y0, y1, z0, z1 = lo(cx, sx), hi(cx, sx, w), lo(cy, sy), hi(cy, sy, h), lo(cz, sz), hi(cz, sz, d)
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    box = (z >= z0) & (z <= z1) & (y >= y0) & (y <= y1) & (x >= x0) & (x <= x1)
    dx, dy, dz = x.astype(np.float64) * sx - cx, y.astype(np.float64) * sy - cy, z.astype(np.float64) * sz - cz
    inside = box & (((dx * dx + dy * dy) + dz * dz) <= radius * radius)
    if edit_mode == 1:
        out[inside & (vol > 0)] = 0
    elif edit_mode == 0:
        if orig is None:
            out[inside] = 255
        else:
            sel = inside & (orig > 0)
            out[sel] = orig[sel]
    return out


def np_filter(size, polygons, edit_mode, polygon2mask):
    """CutMaskFromPolygons:196-200 over a polygon2mask((w, h), points) -> (w, h) bool"""
    w, h = size
    masks = [polygon2mask((w, h), np.asarray(p, np.float64).reshape(-1, 2)) for p in polygons]
    f = np.logical_or.reduce(masks).T if masks else np.zeros((h, w), bool)
    f = np.array(f, bool)
    if edit_mode == 0:
        np.logical_not(f, out=f)
    return f


# ---- matrices -----------------------------------------------------------------------------------------------------------------
def pixel_matrices(shape, spacing, fsize, step=(0.875, 0.9)):
    """(m, mv): voxel x lands on filter column x * step[0] exactly where that product is exact -- column 0 for x = 0, the last
    voxels just below and just past the filter's width -- and mv is the identity, so dist is the voxel's distance from 0"""
    mw, mh = fsize
    sx, sy, sz = spacing
    m = np.zeros((4, 4))
    m[0, 0] = 2.0 * step[0] / (max(mw - 1, 1) * sx)
    m[0, 3] = -1.0
    m[1, 1] = 2.0 * step[1] / (max(mh - 1, 1) * sy)
    m[1, 3] = -1.0
    m[2, 2] = 1.0
    m[3, 3] = 1.0
    return m, np.eye(4)


def perspective_matrices(shape, spacing, eye_z_fraction=0.4):
    """a pinhole inside the volume looking along +z: voxels behind it have q3 <= 0, those in its plane q3 == 0"""
    d, h, w = shape
    sx, sy, sz = spacing
    eye = np.array([(w - 1) * sx / 2.0, -(h - 1) * sy / 2.0,  # (y arrives negated: inv_y stands to the right)
                    round((d - 1) * eye_z_fraction) * sz])
    mv = np.eye(4)
    mv[:3, 3] = -eye
    f = 1.3
    proj = np.array([[f, 0, 0, 0], [0, f, 0, 0], [0, 0, 1.0, -0.1], [0, 0, 1.0, 0]])
    scale = np.diag([1.0 / max((w - 1) * sx, 1.0), 1.0 / max((h - 1) * sy, 1.0), 1.0, 1.0 / max((d - 1) * sz, 1.0)])
    inv_y = np.diag([1.0, -1.0, 1.0, 1.0])
    return scale @ proj @ mv @ inv_y, mv @ inv_y


def ortho_matrices(shape, spacing, fsize):
    """an orthographic camera from outside, through the package's own camera_matrices (Iso view)"""
    from invesalius3_amd import mask3d_editor as M3
    from invesalius3_amd import volume as V

    cam = V.resolve_camera("iso", shape, spacing, fsize)
    return M3.camera_matrices(cam, fsize), cam


def random_filter(fsize, seed=5):
    """an (h, w) filter with both values everywhere"""
    mw, mh = fsize
    rng = np.random.default_rng(seed)
    return rng.random((mh, mw)) < 0.5
