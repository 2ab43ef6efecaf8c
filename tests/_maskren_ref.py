"""A float64 numpy restatement of the mask-preview contract of DESIGN.md section 7e (what csrc/k_maskren.hip computes),
vectorised over rays.  Test infrastructure only: the product never imports it.

    padded(mask, flag)                 the (d + 1)^3 matrix of a dense mask, its index-0 planes holding `flag`
    cells(matrix)                      per 8^3 macro cell (min, max) with a one-voxel apron
    render(matrix, spacing, setup)     a dict: image (H, W, 4), depth, margin, in_box for a volume_mask.render_setup dict

The composite mode is tests/_volren_ref.py's render on the byte field.  The iso mode is restated here on that file's
rays, tri, gradient and headlight; with ``f32=True`` the sample positions and the interpolation run in emulated float32
(the kernel's number format), which is how a test checks, without a GPU, that its inputs keep the two formats' decisions
apart only on the rays it leaves out.
"""
import numpy as np

import _volren_ref as R

ISO = 127.0
CELL = 8


def padded(mask, flag=1):
    m = np.full(tuple(s + 1 for s in mask.shape), flag, np.uint8)
    m[1:, 1:, 1:] = mask
    return m


def cells(matrix):
    return R.cells(matrix).astype(np.uint8)


def render(matrix, spacing, setup, pixels=None, f32=False):
    """`matrix`: the padded uint8 matrix (flag planes included).  Returns {"image": (H, W, 4) float64 (or (len, 4) with
    `pixels`), "in_box": rays that meet the box, and in the iso mode "depth" (inf without a hit) and "margin", the
    smallest |f(t_k) - 127| over a ray's samples up to its hit (inf for a ray without samples)}."""
    w, h = setup["viewport"]
    A, B, hi, tin, kmax = R.rays(matrix.shape, spacing, setup, pixels)
    n = len(tin)
    shape = (h, w) if pixels is None else (n,)
    if not setup["iso"]:
        assert not f32
        return {"image": R.render(matrix, spacing, setup, pixels), "in_box": (kmax >= 0).reshape(shape)}
    ft = np.float32 if f32 else np.float64
    dt = setup["dt"]
    safe_tin = np.where(kmax >= 0, tin, 0.0)
    I0 = (A + safe_tin[:, None] * B[None, :]).astype(ft)  # the kernel's float32 ray: sample 0 and the step per sample
    S = (B * dt).astype(ft)
    hif = hi.astype(ft)

    def pos(idx, k):
        return np.clip(I0[idx] + np.asarray(k, ft)[..., None] * S[None, :], ft(0), hif[None, :])

    bg = np.asarray(setup["background"], np.float64)
    out = np.zeros((n, 4))
    out[:, :3] = bg
    depth = np.full(n, np.inf)
    margin = np.full(n, np.inf)
    live = kmax >= 0
    f_prev = np.zeros(n, ft)
    colour = np.asarray(setup["rgba"][int(ISO), :3], np.float64)
    for k in range(int(kmax.max(initial=-1)) + 1):
        act = np.nonzero(live & (kmax >= k))[0]
        if len(act) == 0:
            break
        p = pos(act, np.full(len(act), k))
        f = R.tri(matrix, p[:, 0], p[:, 1], p[:, 2], ft)
        margin[act] = np.minimum(margin[act], np.abs(f.astype(np.float64) - ISO))
        if k >= 1:
            fp = f_prev[act]
            got = ((fp - ft(ISO)) * (f - ft(ISO)) < 0) | (f == ft(ISO))
            idx = act[got]
            if len(idx):
                fk, fp, pk = f[got], fp[got], p[got]
                pp = pos(idx, np.full(len(idx), k - 1))
                exact = fk == ft(ISO)
                wgt = np.where(exact, ft(1), (ft(ISO) - fp) / np.where(exact, ft(1), fk - fp)).astype(ft)
                ph = np.where(exact[:, None], pk, pp + wgt[:, None] * (pk - pp))
                c = np.repeat(colour[None, :], len(idx), 0)
                if setup["shade"]:
                    c = R.headlight(matrix, ph[:, 0], ph[:, 1], ph[:, 2], hif, spacing, setup, c, ft)
                out[idx, :3] = c
                out[idx, 3] = 1.0
                depth[idx] = tin[idx] + ((k - 1) + wgt.astype(np.float64)) * dt
                live[idx] = False
        f_prev[act] = f
    img_shape = (h, w, 4) if pixels is None else (n, 4)
    return {"image": out.reshape(img_shape), "depth": depth.reshape(shape), "margin": margin.reshape(shape),
            "in_box": (kmax >= 0).reshape(shape)}


def position_bound(matrix_shape, spacing, setup):
    """The a-priori float32 error of a sample's index position: the position is I0 + float(k) S, three roundings of
    quantities no larger than the index extent, for sample counts k up to kmax, so at most
    extent x (samples) x 2^-24 index units -- a deliberately loose figure, the rounding of I0 and S themselves taken
    as growing with k.  Returns (bound in index units, sample count)."""
    sx, sy, sz = [float(s) for s in spacing]
    nz, ny, nx = matrix_shape
    extent = max(nz, ny, nx)
    diag = np.sqrt(((nx - 1) * sx) ** 2 + ((ny - 1) * sy) ** 2 + ((nz - 1) * sz) ** 2)
    count = int(np.floor(diag / setup["dt"])) + 1
    return extent * count * 2.0 ** -24, count


def max_slope(matrix):
    """The largest slope of the trilinear field per index unit: along one axis it is at most the largest difference of
    two neighbouring voxels on that axis; along a ray the three axes add."""
    m = matrix.astype(np.int64)
    s = 0
    for a in range(3):
        if m.shape[a] > 1:
            s += int(np.abs(np.diff(m, axis=a)).max())
    return float(s)


# -- inputs the CPU and the GPU tests share ---------------------------------------------------------------------------
def thresholded(img, lo=226, hi=3071):
    return (((img >= lo) & (img <= hi)) * 255).astype(np.uint8)


def levels_mask(shape, seed=5):
    """a mask that holds 0 / 1 / 2 / 253 / 254 / 255 in blocks, as edits, region growing and watershed leave them"""
    rng = np.random.default_rng(seed)
    coarse = rng.choice(np.array([0, 0, 1, 2, 253, 254, 255], np.uint8), size=[-(-s // 4) for s in shape])
    m = np.kron(coarse, np.ones((4, 4, 4), np.uint8))[:shape[0], :shape[1], :shape[2]]
    return np.ascontiguousarray(m)


def case_masks():
    """name -> dense uint8 mask: thresholded volumes with material on the faces, the byte levels, empty and full"""
    out = {"ct": thresholded(R.cropped_ct((22, 30, 36), seed=11)),
           "synth": thresholded(R.synth_volume((24, 28, 32), seed=3, shell=0)),
           "levels": levels_mask((20, 24, 28)),
           "empty": np.zeros((9, 10, 11), np.uint8),
           "full": np.full((9, 10, 11), 255, np.uint8)}
    return out


def compare_mask(ref, eps):
    """the rays an iso comparison keeps: inside the box and with a margin of at least eps"""
    return ref["in_box"] & (ref["margin"] >= eps)


def noise_gradients(matrix, spacing, setup, floor=1e-3):
    """How many samples a composite ray colours (f > 0, up to its first opaque sample) at which the central differences
    are not zero yet below `floor`: there the true gradient is zero and the shading's N = g / |g| is the direction of
    rounding noise, in float64 as much as in float32 (a difference of two bytes' interpolations is either 0 or far above
    1e-3 unless it is noise: the field's slopes are whole bytes per voxel).  An input for a colour comparison has none."""
    A, B, hi, tin, kmax = R.rays(matrix.shape, spacing, setup)
    I0 = A + np.where(kmax >= 0, tin, 0.0)[:, None] * B[None, :]
    S = B * setup["dt"]
    live = kmax >= 0
    count = 0
    for k in range(int(kmax.max(initial=-1)) + 1):
        act = np.nonzero(live & (kmax >= k))[0]
        if len(act) == 0:
            break
        p = np.clip(I0[act] + k * S[None, :], 0.0, hi[None, :])
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        gx, gy, gz = R.gradient(matrix, x, y, z, hi)
        gn = np.sqrt(gx * gx + gy * gy + gz * gz)
        f = R.tri(matrix, x, y, z)
        count += int(np.count_nonzero((gn > 0) & (gn < floor) & (f > 0)))
        live[act[f >= ISO]] = False  # opacity 1 from 127 on: the ray ends
    return count


def space_mask():
    """material (byte levels around a solid core) with empty space on every side"""
    mask = np.zeros((40, 44, 48), np.uint8)
    mask[12:30, 10:30, 16:40] = levels_mask((20, 24, 28))[:18, :20, :24]
    mask[14:28, 14:26, 20:36] = 255
    return mask


def gpu_iso_inputs():
    """(id, padded matrix, spacing, view, size, render_setup keywords) of every iso comparison against the oracle in
    tests/test_gpu_volume_mask.py, so that the CPU can check them in emulated float32 before a GPU does"""
    sp, size, sweep = (0.8, 0.9, 1.2), (48, 40), (21, 19)
    c = case_masks()
    out = [("ct-" + v, padded(c["ct"]), sp, v, size, {}) for v in ("front", "back", "left", "right", "top", "bottom", "iso")]
    for name, view, s in (("synth", "iso", sp), ("synth", "left", (0.4, 1.7, 0.9)), ("levels", "iso", sp),
                          ("levels", "bottom", (0.4, 1.7, 0.9)), ("levels", "front", sp)):
        out.append(("%s-%s-%g" % (name, view, s[0]), padded(c[name]), s, view, size, {}))
    for name in ("empty", "full"):
        out += [("%s-%s" % (name, v), padded(c[name]), sp, v, size, {"background": (0.25, 0.5, 0.75)}) for v in ("iso", "back")]
    for shape in [(1, 20, 23), (2, 9, 17), (9, 8, 7), (17, 3, 16), (12, 33, 1), (8, 8, 8), (3, 17, 2), (16, 1, 9), (6, 2, 3)]:
        m = padded(thresholded(R.cropped_ct(shape, seed=sum(shape)), 200, 3071))
        out += [("%dx%dx%d-%s" % (shape + (v,)), m, (0.9, 0.7, 1.1), v, sweep, {}) for v in ("front", "top", "right", "iso")]
    out.append(("ct-dt0.25", padded(c["ct"]), sp, "iso", size, {"sample_distance": 0.25}))
    m = padded(c["ct"], 0)
    m[1:, 0, 0], m[3:9, 0, 0], m[0, 4:11, 0], m[0, 0, 2:20] = 1, 2, 2, 2
    out += [("mixed-" + v, m, sp, v, size, {}) for v in ("iso", "front", "top")]
    out += [("space-" + v, padded(space_mask()), sp, v, (64, 56), {}) for v in ("iso", "back")]
    return out
