"""Case tables and plain references for the small streaming kernels (k_mip, k_misc, k_edit, k_area, k_holes, k_jump,
k_synth): the launch arithmetic of the host code restated in Python, so that every case can say which branch it takes, and
numpy / Python-int references of what the kernels compute.  Nothing here imports the package under test; the restated
constants are the ones the .hip files hold (a retune shows up in test_stream_cases_host.py, not as a silently untested path).
"""
import math
from fractions import Fraction

import numpy as np

I16_MIN, I16_MAX = -32768, 32767


def cdiv(a, b):
    return -(-a // b)


# ---- k_mip.hip: run_reduce's split of a strided ray (axis 0 / 1) ---------------------------------------------------------
MIP_TARGET_BLOCKS, MIP_MIN_SEG, MIP_MAX_SEG = 2048, 32, 32767


def mip_split_plan(nr, nc, length, itemsize):
    """(nblk, first split, split, seg, last segment) of run_reduce<T, OP> for an (nr, nc) output of rays `length` long:
    `first split` is the value before seg = cdiv(len, split) and the recomputation split = cdiv(len, seg)."""
    vec = 16 // itemsize
    nblk = cdiv(nr * cdiv(nc, vec), 256)
    split = cdiv(MIP_TARGET_BLOCKS, nblk)
    if split > length // MIP_MIN_SEG:
        split = length // MIP_MIN_SEG
    if split < cdiv(length, MIP_MAX_SEG):
        split = cdiv(length, MIP_MAX_SEG)
    if split < 1:
        split = 1
    first = split
    seg = cdiv(length, split)
    split = cdiv(length, seg)
    return dict(nblk=nblk, first=first, split=split, seg=seg, last=length - (split - 1) * seg)


def mip_plan_of(shape, axis, itemsize=2):
    dz, dy, dx = shape
    nr, nc, length = ((dy, dx, dz), (dz, dx, dy))[axis]
    return mip_split_plan(nr, nc, length, itemsize)


# id, slab shape for axis 0, what the plan must be (None: not asserted)
MIP_SPLIT_CASES = [
    ("mip-split1-len1", (1, 3, 8), dict(nblk=1, split=1)),
    ("mip-split1-len31", (31, 3, 8), dict(nblk=1, split=1)),
    ("mip-split1-len32", (32, 3, 8), dict(nblk=1, split=1)),
    ("mip-split1-len63", (63, 3, 8), dict(nblk=1, split=1)),
    ("mip-split2-seg32-len64", (64, 3, 8), dict(nblk=1, split=2, seg=32, last=32)),
    ("mip-split2-seg33-len65", (65, 3, 8), dict(nblk=1, split=2, seg=33, last=32)),
    ("mip-split3-seg33-last31-len97", (97, 3, 8), dict(nblk=1, split=3, seg=33, last=31)),
    ("mip-split4-seg33-last30-len129", (129, 3, 8), dict(nblk=1, split=4, seg=33, last=30)),
    ("mip-split-2048to2000", (70000, 3, 8), dict(nblk=1, first=2048, split=2000, seg=35, last=35)),
    ("mip-nblk12-split2", (70, 600, 40), dict(nblk=12, split=2, seg=35, last=35)),
]


def mip_slab(shape, seed, dtype=np.int16):
    """full-range noise with both ends of the dtype present in the first ray"""
    info = np.iinfo(dtype)
    a = np.random.default_rng(seed).integers(info.min, info.max + 1, shape).astype(dtype)
    a.reshape(-1)[0] = info.min
    a.reshape(-1)[-1] = info.max
    return a


MIP_U8_WIDTHS = (15, 16, 17, 33)                 # one lane owns 16 adjacent uint8 pixels
MIP_ROW_LENGTHS = (1, 7, 8, 9, 511, 512, 513)    # axis 2: 8 int16 per 16-byte load


def mip_rows_branch(ray, length, itemsize=2, base_offset=0):
    """k_reduce_rows for one ray: 'vec' / 'vec+tail' when its first element is 16-byte aligned, else 'scalar'"""
    if (base_offset + ray * length * itemsize) % 16:
        return "scalar"
    vec = 16 // itemsize
    if length < vec:
        return "vec0+tail"  # aligned, but the vector loop has no full chunk: the tail loop does everything
    return "vec+tail" if length % vec else "vec"


# ---- k_mip.hip: viewport replication --------------------------------------------------------------------------------------
REPLICATE_CASES = [(5, 8, 1), (3, 4, 2), (16, 16, 4), (2, 6, 4), (3, 5, 1), (7, 3, 3), (3, 3, 1), (1, 1, 1), (1, 1, 7), (9, 5, 3)]


def replicate_branch(h, w, f):
    """dict(fast, straddles, partial): the 16-byte store path, whether an 8-pixel chunk spans two output rows, whether the
    last chunk is shorter than 8"""
    W, total = w * f, h * f * w * f
    fast = W % 8 == 0
    straddles = (not fast) and any((i % W) + min(8, total - i) > W for i in range(0, total, 8))
    return dict(fast=fast, straddles=straddles, partial=total % 8 != 0)


def replicate_id(h, w, f):
    b = replicate_branch(h, w, f)
    tag = "fast" if b["fast"] else "ragged" + ("-straddle" if b["straddles"] else "") + ("-partial" if b["partial"] else "")
    return "replicate-%s-%dx%dx%d" % (tag, h, w, f)


def replicate_src(h, w, seed=0):
    a = np.random.default_rng(700 + seed).integers(I16_MIN, I16_MAX + 1, (h, w)).astype(np.int16)
    a[0, 0] = I16_MIN
    a[-1, -1] = I16_MAX if a.size > 1 else a[-1, -1]
    return a


def replicate_ref(src, f):
    return np.repeat(np.repeat(src, f, 0), f, 1)


# ---- the `vec` switches of k_misc.hip ---------------------------------------------------------------------------------------
VEC_N = (1, 7, 8, 9, 15, 16, 17, 4099)
I16_OFFS, U8_OFFS = (2, 6, 14), (1, 7, 9)
# kernel -> (pointers: (name, alignment the host code tests, offsets to try), n below which the scalar body runs, voxels per lane)
VEC_KERNELS = {
    "lut": ((("img", 16, I16_OFFS), ("out", 16, I16_OFFS)), 8, 8),
    "merge": ((("mask", 16, U8_OFFS), ("tmp", 16, U8_OFFS)), 16, 16),
    "boolean": ((("m1", 16, U8_OFFS), ("m2", 16, U8_OFFS), ("out", 16, U8_OFFS)), 16, 16),
    "density": ((("img", 16, I16_OFFS), ("mask", 8, U8_OFFS + (4,))), 8, 8),
}


def vec_branch(kernel, n, offs):
    """'scalar', 'vec' or 'vec+tail' for `n` elements and byte offsets {pointer name: offset} from a 256-byte aligned base"""
    ptrs, min_n, chunk = VEC_KERNELS[kernel]
    if n < min_n or any(offs.get(name, 0) % align for name, align, _ in ptrs):
        return "scalar"
    return "vec+tail" if n % chunk else "vec"


def vec_cases(kernel):
    """[(id, n, {pointer: offset})]: every n with aligned bases, then with each pointer offset in turn"""
    ptrs = VEC_KERNELS[kernel][0]
    out = []
    for n in VEC_N:
        combos = [{}] + [{name: o} for name, _, offs in ptrs for o in offs]
        for offs in combos:
            where = "aligned" if not offs else "%soff%d" % next(iter(offs.items()))
            out.append(("%s-%s-n%d-%s" % (kernel, vec_branch(kernel, n, offs), n, where), n, offs))
    return out


MASK_BYTES = np.array([0, 127, 128, 255], np.uint8)
MERGE_MASK_BYTES = np.array([0, 1, 2, 253, 254, 255, 7], np.uint8)


def boolean_ref(op, a, b):
    """Slice.do_boolean_op's numpy expressions (slice_.py:1906-1916)"""
    return {1: ((a > 2) + (b > 2)) * 255, 2: ((a > 2) ^ ((a > 2) & (b > 2))) * 255, 3: ((a > 2) & (b > 2)) * 255,
            4: np.logical_xor((a > 2), (b > 2)) * 255}[op].astype(np.uint8)


def int_sums(vals):
    """(count, sum, sum of squares) of an integer array as Python ints"""
    v = np.asarray(vals).ravel().tolist()  # Python ints
    return len(v), sum(v), sum(x * x for x in v)


def density_ref(img, sel):
    """(count, sum, sum of squares, min, max) of img[sel] as Python ints; min / max are 32767 / -32768 for an empty selection,
    which is how the device initialises them"""
    vals = img[sel]
    cnt, s1, s2 = int_sums(vals)
    return cnt, s1, s2, (int(vals.min()) if cnt else I16_MAX), (int(vals.max()) if cnt else I16_MIN)


# ---- LUT and min-shift over the whole int16 domain ---------------------------------------------------------------------------
LUT_WINDOWS = [(1, 0), (2, 0), (255, 127), (80.5, 40.25), (32767, 0), (400, -32768), (400, 32767)]  # (ww, wl)


def all_int16(shape=(4, 128, 128)):
    a = np.arange(I16_MIN, I16_MAX + 1, dtype=np.int32).astype(np.int16)
    return np.random.default_rng(16).permutation(a).reshape(shape)


def min_shift_ref(img):
    return (img - img.min()).astype("uint16")  # watershed_process.py:47


# ---- exact variance ------------------------------------------------------------------------------------------------------------
def exact_std(vals):
    """sqrt of the exact rational variance, rounded once to float64 and once by sqrt"""
    cnt, s1, s2 = int_sums(vals)
    return math.sqrt(float(Fraction(cnt * s2 - s1 * s1, cnt * cnt)))


def float_formula_std(vals):
    """sqrt(E[x^2] - mean^2) in float64 from the exact sums: what calc_image_density did before"""
    cnt, s1, s2 = (float(v) for v in int_sums(vals))
    mean = s1 / cnt
    return math.sqrt(max(s2 / cnt - mean * mean, 0.0))


STD_CASES = [("std-100000x1000-one-1001", 1000, 1001), ("std-100000x32766-one-32767", 32766, 32767), ("std-constant", -700, -700)]


def std_case(base, odd, shape=(10, 101, 100)):
    """image + padded mask: the mask selects 100,000 voxels of `base` and one of `odd`; the rest of the image is noise"""
    rng = np.random.default_rng(abs(base))
    img = rng.integers(-1024, 3072, shape).astype(np.int16)
    sel = np.zeros(img.size, bool)
    sel[rng.permutation(img.size)[:100001]] = True
    sel = sel.reshape(shape)
    img[sel] = base
    z, y, x = np.argwhere(sel)[50000]
    img[z, y, x] = odd
    m = np.zeros(tuple(s + 1 for s in shape), np.uint8)
    m[1:, 1:, 1:] = np.where(sel, rng.choice(np.array([128, 255], np.uint8), shape), rng.choice(np.array([0, 127], np.uint8), shape))
    return img, m


# ---- k_edit.hip ------------------------------------------------------------------------------------------------------------------
COUNT_LDS_BINS, COUNT_GRID_CAP = 4096, 2048


def count_branch(nreg):
    return "lds" if nreg < COUNT_LDS_BINS else "global"


def count_hist_launch(n):
    """(blocks, trips of the histogram loop)"""
    blocks = max(1, min(cdiv(n, 1024), 16384, COUNT_GRID_CAP))
    return blocks, cdiv(n, blocks * 256)


def count_labels(n, nreg, dtype, seed=0):
    """n labels in [0, nreg]; every bin at least once when n > nreg.  Shape (1, 1, n)."""
    rng = np.random.default_rng(900 + seed)
    lab = rng.integers(0, nreg + 1, n)
    if n > nreg:
        lab[rng.permutation(n)[:nreg + 1]] = np.arange(nreg + 1)
    return lab.astype(dtype).reshape(1, 1, n)


def _count_cases():
    out = []
    for nreg in (4094, 4095, 4096, 4097, 70000):
        for dt in (np.int16, np.int32, np.int64):
            if nreg > np.iinfo(dt).max:
                continue
            out.append(("count-%s-%d-%s" % (count_branch(nreg), nreg, np.dtype(dt).name), nreg + 518, nreg, dt))
    for nreg in (7, 4096):
        for n in (1, 63, 257):
            out.append(("count-%s-%d-n%d" % (count_branch(nreg), nreg, n), n, nreg, np.int32))
    out.append(("count-lds-300-n1100000-4trips", 1100000, 300, np.int32))
    out.append(("count-global-5000-n2200000-capped-grid-5trips", 2200000, 5000, np.int32))
    return out


COUNT_CASES = _count_cases()  # (id, n, nreg, dtype)

CUT_SHAPES = [(5, 4, 1), (2, 1, 17), (1, 1, 16), (3, 5, 16), (1, 3, 5)]
CUT_SPACING = (0.5, 0.75, 1.25)


def cut_branch(shape):
    n = shape[0] * shape[1] * shape[2]
    return "scalar" if n < 16 else ("vec+tail" if n % 16 else "vec")


def cut_camera(shape, spacing=CUT_SPACING):
    """(m, mv, max_depth): a perspective camera whose eye sits inside the volume, so part of it is behind the eye
    (q3 <= 0), and a depth limit at the median eye distance, which cuts through the rest"""
    d, h, w = shape
    ext = np.array([(w - 1) * spacing[0], (h - 1) * spacing[1], (d - 1) * spacing[2]])
    eye = ext / 2.0 + np.array([0.11, 0.07, 0.05])
    f = np.array([1.0, 0.6, 0.8])
    f /= np.linalg.norm(f)
    s = np.cross(f, [0.0, 1.0, 0.0])
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = s, u, -f
    view[:3, 3] = -view[:3, :3] @ eye
    near, far, t = 0.1, 100.0, 0.5
    proj = np.array([[1 / t, 0, 0, 0], [0, 1 / t, 0, 0], [0, 0, -(far + near) / (far - near), -2 * far * near / (far - near)],
                     [0, 0, -1, 0]])
    m, mv = np.ascontiguousarray(proj @ view), np.ascontiguousarray(view)
    g = cut_geometry(shape, spacing, m, mv)
    return m, mv, float(np.median(g["dist"]))


def cut_geometry(shape, spacing, m, mv):
    """q3, the eye distance and the screen position (in [-1, 1]) of every voxel, in numpy: for choosing and checking cases"""
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    p = np.stack([x * spacing[0], y * spacing[1], z * spacing[2], np.ones(x.shape)], -1).reshape(-1, 4).astype(np.float64)
    q = p @ m.T
    c = p @ mv.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(q3=q[:, 3], dist=np.linalg.norm(c[:, :3] / c[:, 3:4], axis=1), sx=q[:, 0] / q[:, 3], sy=q[:, 1] / q[:, 3])


def cut_mask(shape, seed=0):
    return np.random.default_rng(40 + seed).choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), size=shape,
                                                   p=[0.1, 0.05, 0.05, 0.2, 0.2, 0.4])


def cut_screen(kind):
    if kind == "1x1":
        return np.ones((1, 1), bool)
    s = np.random.default_rng(41).random((6, 7)) < 0.6
    s[0, 0] = True
    return s


# (id, shape, spacing, centre (x, y, z), radius)
BRUSH_CASES = [
    ("brush-on-voxel-integer-radius", (9, 9, 9), (1.0, 1.0, 1.0), (4.0, 4.0, 4.0), 3.0),
    ("brush-centre-past-far-faces-clipped-box", (9, 9, 9), (1.0, 1.0, 1.0), (12.0, 11.0, 10.0), 6.0),
    ("brush-centre-past-far-faces-empty-box", (9, 9, 9), (1.0, 1.0, 1.0), (30.0, 30.0, 30.0), 3.0),
    ("brush-anisotropic", (7, 20, 12), (0.5, 0.25, 2.0), (3.0, 2.5, 6.0), 2.5),
]


def brush_dist_sq(shape, spacing, centre):
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    dx, dy, dz = x * spacing[0] - centre[0], y * spacing[1] - centre[1], z * spacing[2] - centre[2]
    return (dx * dx + dy * dy) + dz * dz


# ---- k_area.hip ------------------------------------------------------------------------------------------------------------------
AREA_VOXELS_PER_BLOCK = 2048
AREA_EXACT_SPACINGS = [(1.0, 1.0, 1.0), (0.5, 0.25, 2.0)]  # every face area is a multiple of 1/8: sums are exact in any order
AREA_INEXACT_SPACING = (0.4785156, 0.4785156, 2.0)
# (id, interior shape)
AREA_SHAPES = [("area-one-block-210", (5, 6, 7)), ("area-2047-one-block", (1, 23, 89)), ("area-2048-one-full-block", (8, 16, 16)),
               ("area-2049-two-blocks", (3, 683, 1)), ("area-extent1-z", (1, 5, 6)), ("area-extent1-y", (5, 1, 6)),
               ("area-extent1-x", (5, 6, 1))]


def area_mask(interior, seed=0):
    m = np.zeros(tuple(s + 1 for s in interior), np.uint8)
    m[1:, 1:, 1:] = np.random.default_rng(50 + seed).choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), size=interior)
    return m


CONVOLVE_GRID_CAP = 16384


# ---- k_holes.hip: Mask.fill_holes_auto ---------------------------------------------------------------------------------------------
HOLES_SHAPE = (3, 5, 70)  # interior; a row is two 64-bit words of the bit plane


def holes_case(kind):
    """(padded matrix, max_size): a: five selected voxels in one big background, max_size = their count -- label 0 alone is
    small; b: the same plus one background voxel walled in by six selected ones; c: as a with max_size one below the count"""
    m = np.zeros(tuple(s + 1 for s in HOLES_SHAPE), np.uint8)
    inner = m[1:, 1:, 1:]
    for z, y, x in ((0, 0, 0), (1, 2, 10), (2, 4, 69), (1, 1, 63), (1, 1, 64)):
        inner[z, y, x] = 255
    if kind == "b":
        z, y, x = 1, 3, 65
        for dz, dy, dx in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            inner[z + dz, y + dy, x + dx] = 200
    selected = int((inner > 127).sum())
    return m, (selected - 1 if kind == "c" else selected)


# ---- k_misc.hip: fill_holes_automatically with explicit labels ---------------------------------------------------------------------
def label_volume(nlabels, seed=0):
    """uint32 labels (2, 8, 64): the first 64 voxels share one label (one atomic for the wave), the next 64 all differ (one
    atomic per lane), the rest is random in [0, nlabels] with `nlabels` itself present"""
    rng = np.random.default_rng(60 + seed)
    lab = rng.integers(0, nlabels + 1, 2 * 8 * 64).astype(np.uint32)
    lab[lab == 5] = 6
    lab[:64] = 5
    lab[64:128] = np.arange(100, 164)
    lab[-1] = nlabels
    return lab.reshape(2, 8, 64)


# ---- k_jump.hip ------------------------------------------------------------------------------------------------------------------
JF_LDS_SITES = 1024


def jump_steps(shape):
    m, n = max(shape), 0
    if m > 1:
        while (m >> (n + 1)) > 0:
            n += 1
    return n


def jump_sites(shape, nsites, seed=0):
    """distinct voxels of `shape` as (n, 3) int32 rows of (z, y, x)"""
    total = shape[0] * shape[1] * shape[2]
    flat = np.random.default_rng(70 + seed).permutation(total)[:nsites]
    return np.stack(np.unravel_index(flat, shape), 1).astype(np.int32)


# (id, shape, number of sites, normalize)
JUMP_CASES = [("jump-normalise-lds-1024", (8, 16, 32), 1024, True), ("jump-normalise-global-1025", (8, 16, 32), 1025, True),
              ("jump-0passes-1x1x1", (1, 1, 1), 1, False), ("jump-0passes-1x1x1-normalise", (1, 1, 1), 1, True),
              ("jump-1pass-odd-1x1x2", (1, 1, 2), 1, False), ("jump-1pass-odd-1x1x2-normalise", (1, 1, 2), 2, True),
              ("jump-1pass-odd-2x3x1", (2, 3, 1), 2, False), ("jump-1pass-odd-2x3x1-normalise", (2, 3, 1), 2, True)]


# ---- k_synth.hip -------------------------------------------------------------------------------------------------------------------
SYNTH_SEED = 20260924
_M32 = np.uint64(0xFFFFFFFF)


def synth_blobs(seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.15, 0.85, 6), rng.uniform(0.15, 0.85, 6), rng.uniform(0.15, 0.85, 6), rng.uniform(0.12, 0.28, 6)],
                    axis=1).astype(np.float32)  # (cz, cy, cx, sigma) x 6


def _mix32(x):
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M32
    return x ^ (x >> np.uint64(16))


def synth_hash(g, seed):
    """(h1, h2) of the global voxel index g (uint64 array): integer arithmetic mod 2^32, exactly the kernel's"""
    g = np.asarray(g, np.uint64)
    h1 = _mix32((g & _M32) ^ np.uint64(seed))
    h2 = _mix32(((g >> np.uint64(32)) * np.uint64(0x9E3779B9) + h1 + np.uint64(0x85ebca6b)) & _M32)
    return h1, h2


def synth_hash_py(g, seed):
    """the same with Python ints, one index"""
    def mix(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        return x ^ (x >> 16)
    h1 = mix((g & 0xFFFFFFFF) ^ seed)
    return h1, mix(((g >> 32) * 0x9E3779B9 + h1 + 0x85ebca6b) & 0xFFFFFFFF)


def synth_field(shape, z0, z_total, seed, blobs, dtype=np.float64):
    """the recipe of k_synth.hip before the clip and the truncation, evaluated in `dtype` throughout (float32: the kernel's
    own operation order with numpy's accurate exp / sin / cos / log in place of the fast intrinsics)"""
    F = np.dtype(dtype).type
    dz, dy, dx = shape
    z, y, x = np.meshgrid(np.arange(z0, z0 + dz), np.arange(dy), np.arange(dx), indexing="ij")
    fz = z.astype(F) / F(max(z_total - 1, 1))
    fy = y.astype(F) / F(max(dy - 1, 1))
    fx = x.astype(F) / F(max(dx - 1, 1))
    b = np.asarray(blobs, np.float32).astype(F)
    f = np.zeros(shape, F)
    for cz, cy, cx, s in b:
        inv2s2 = F(1) / (F(2) * s * s)
        d2 = (fz - cz) * (fz - cz) + (fy - cy) * (fy - cy) + (fx - cx) * (fx - cx)
        f = f + F(1800) * np.exp(-d2 * inv2s2)
    f = f + F(150) * np.sin(F(6) * fx) * np.cos(F(5) * fz) * np.cos(F(4) * fy)
    g = ((z * dy + y) * dx + x).astype(np.uint64)
    h1, h2 = synth_hash(g, seed)
    u1 = ((h1 >> np.uint64(8)).astype(F) + F(1)) * (F(1) / F(16777217))
    u2 = (h2 >> np.uint64(8)).astype(F) * (F(1) / F(16777216))
    f = f + F(25) * np.sqrt(F(-2) * np.log(u1)) * np.cos(F(6.2831853) * u2)
    f = f - F(1000)
    assert f.dtype == np.dtype(dtype)
    return f


def synth_clip(f):
    return np.clip(f, -1024.0, 3071.0)


def synth_tolerance(shape):
    """1 HU for the truncation + the float32-vs-float64 spread of the recipe itself on this case, rounded up"""
    blobs = synth_blobs()
    f64 = synth_field(shape, 0, shape[0], SYNTH_SEED, blobs, np.float64)
    f32 = synth_field(shape, 0, shape[0], SYNTH_SEED, blobs, np.float32)
    return 1 + int(math.ceil(float(np.abs(f32.astype(np.float64) - f64).max())))


SYNTH_CASES = [("synth-12x9x20", (12, 9, 20)), ("synth-dy1", (5, 1, 33)), ("synth-dx1", (5, 7, 1))]
