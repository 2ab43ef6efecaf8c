"""Named cases for the ordered ray projections (csrc/k_rays.hip: MIDA, LMIP, the fused contour MaxIP, MIDA's min / max pre-pass)
where the volumes of test_gpu_rays.py do not reach: ray lengths on both sides of the 16-sample blocks of k_rays_strided, rows on
both sides of the LDS chunks of k_rays_rows with aligned and unaligned pointers, waves with dead lanes, rays that end where they
are told to, every FAST variant of ivx_dev_fcm_maxip, ragged and 32-fold segment splits, pixels the bounds must leave open, and
the vector body / scalar tail / block cap of k_minmax_part.  Pure numpy: nothing here imports the package under test or the
oracle.  Each case carries the branch it claims to reach; test_ray_cases_host.py proves the claims without a device.

Two kinds of restatement live here, both read off k_rays.hip:
  * which branch a call takes (strided_plan, staged_plan, fcm_plan, minmax_plan): integer arithmetic, exact;
  * the decide rule of k_fcm_max_decide on the bounds of fcm_lin_fold / fcm_pow_fold / fcm_value_fast (classify), in float32
    numpy.  numpy's root, reciprocal root, log2 and exp2 are not the transcendental unit's, so a bound restated here can differ
    from the device's in its last bits: classify is NOT a second reference for the picture.  It says whether a pixel is decided
    or open and which segments stay open, and the forced-open cases keep three orders of magnitude between the bound (1e-5) and
    the distances that decide their classification (0.4 and more), so the last bits cannot change the answer.
"""
from collections import namedtuple

import numpy as np

F = np.float32
I16, U8, F64 = np.dtype(np.int16), np.dtype(np.uint8), np.dtype(np.float64)
DTYPES = (I16, U8, F64)


def cdiv(a, b):
    return -(-int(a) // int(b))


# ================================================================================================================================
# which branch a call takes
# ================================================================================================================================
B = 16  # samples per block of k_rays_strided


def strided_plan(length):
    """k_rays_strided for a ray of `length` samples none of which ends early: (iterations of the unguarded loop, blocks of the
    guarded loop).  The unguarded loop runs while l0 + 2 B <= len, the guarded one takes what is left from l0 on."""
    l0 = unguarded = 0
    while l0 + 2 * B <= length:
        unguarded += 1
        l0 += B
    return unguarded, cdiv(length - l0, B) if length > l0 else 0


StagedPlan = namedtuple("StagedPlan", "CH PER vec_ok chunks last_chunk words tail waves last_wave_live")


def staged_plan(length, itemsize, offset_bytes, nrays):
    """k_rays_rows: CH elements per staged chunk, PER samples per 8-byte LDS read, the 16-byte load path, the number of chunks,
    the last chunk's length, its whole words and its scalar tail, the waves and the live lanes of the last one"""
    CH, PER = 128 // itemsize, 8 // itemsize
    chunks = cdiv(length, CH)
    last = length - (chunks - 1) * CH
    waves = cdiv(nrays, 64)
    return StagedPlan(CH, PER, (length * itemsize) % 16 == 0 and offset_bytes % 16 == 0, chunks, last, last // PER, last % PER,
                      waves, nrays - (waves - 1) * 64)


MinmaxPlan = namedtuple("MinmaxPlan", "V body tail blocks strides")


def minmax_plan(n, itemsize, offset_bytes):
    """k_minmax_part: V elements per 16-byte load, elements in the vector body (0 at an unaligned pointer), elements in the
    scalar tail, blocks (capped at 2048), and how often the busiest lane goes round its grid-stride loop in the scalar part"""
    V = 16 // itemsize
    body = (n // V) * V if offset_bytes % 16 == 0 else 0
    blocks = min(cdiv(n, 256), 2048)
    return MinmaxPlan(V, body, n - body, blocks, cdiv(n - body, blocks * 256))


FcmPlan = namedtuple("FcmPlan", "route pmode lin fast unit FAST nblk split seg last_seg")


def fcm_plan(shape, axis, n, dtype=I16, offset_bytes=0):
    """ivx_dev_fcm_maxip's dispatch with none of its environment switches set.  route: "fused" or "materialised" (the contour
    volume + MaxIP); pmode 1 = exponent 1, 2 = glibc's powf (either build); FAST 0 exact fold + combine, 1 bounds of the power
    (0 < n < 1), 2 exponent 1, 3 the unit's root in front of the fast power (1 < n <= 64)."""
    dz, dy, dx = shape
    n = F(n)
    pmode = 1 if n == F(1.0) else 2
    if not (np.dtype(dtype) == I16 and dx % 8 == 0 and offset_bytes % 16 == 0):
        return FcmPlan("materialised", pmode, False, False, False, None, None, None, None, None)
    lin = pmode == 1
    fast = lin or (F(0.0) < n <= F(64.0))
    unit = (not lin) and fast and n >= F(1.0)
    FAST = 2 if lin else 3 if unit else 1 if fast else 0
    if axis == 2:
        return FcmPlan("fused", pmode, lin, fast, unit, FAST, cdiv(dz * dy, 4), 1, dx, dx)
    nr, length = (dy, dz) if axis == 0 else (dz, dy)
    nblk = cdiv(nr * (dx // 8), 256)
    split = cdiv(1024 if lin else 2048, nblk)
    split = max(1, min(split, length // 32, 32))
    seg = cdiv(length, split)
    split = cdiv(length, seg)
    return FcmPlan("fused", pmode, lin, fast, unit, FAST, nblk, split, seg, length - (split - 1) * seg)


# ================================================================================================================================
# the decide rule of k_fcm_max_decide, restated
# ================================================================================================================================
def wrapped_diffs(vol):
    """the central differences of an int16 volume with clamped ends, taken in int16 and wrapping like the reference's
    T-subtraction: (Dz, Dy, Dx) as int32"""
    out = []
    for ax in range(3):
        k = np.arange(vol.shape[ax])
        fwd = np.take(vol, np.minimum(k + 1, k[-1]), axis=ax).astype(np.int32)
        bwd = np.take(vol, np.maximum(k - 1, 0), axis=ax).astype(np.int32)
        out.append((fwd - bwd).astype(np.int16).astype(np.int32))
    return out


def _pow_fast(base, n):
    """fcm_pow_fast: (2 ** (n * log2(base)), relative bound)"""
    base = base.astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = (F(n) * np.log2(base)).astype(F)
        p = np.exp2(y).astype(F)
    rel = ((np.abs(y) + F(4.0)) * F(4.76837158203125e-7)).astype(F)
    gone = ~(y > F(-160.0))
    p, rel = np.where(gone, F(0.0), p), np.where(gone, F(0.0), rel)
    p, rel = np.where(base >= F(1.0), F(1.0), p), np.where(base >= F(1.0), F(0.0), rel)
    p, rel = np.where(base <= F(0.0), F(0.0), p), np.where(base <= F(0.0), F(0.0), rel)
    return p.astype(F), rel.astype(F)


Classified = namedtuple("Classified", "open mask lo hi plan")


def classify(vol, n, axis):
    """Every pixel of ivx_dev_fcm_maxip(vol, n, axis) on the fused fast routes: open (handed to k_fcm_fix) or decided, the word
    of open segments, and the pixel's bounds.  Arrays have the picture's shape."""
    plan = fcm_plan(vol.shape, axis, n)
    assert plan.route == "fused" and plan.fast, "the decide rule runs on the fused fast routes only"
    dzyx = wrapped_diffs(vol)
    dray = np.moveaxis(dzyx[axis], axis, 0)
    others = [np.moveaxis(dzyx[a], axis, 0) for a in range(3) if a != axis]
    S = (dray.astype(np.int64) ** 2 + others[0].astype(np.int64) ** 2 + others[1].astype(np.int64) ** 2)
    assert S.max() < 2 ** 32
    Sf = S.astype(F)
    split, seg, length = plan.split, plan.seg, dray.shape[0]
    cuts = [(s * seg, min((s + 1) * seg, length)) for s in range(split)]
    n = F(n)
    if plan.lin:  # fcm_lin_fold: t = root(S) - |Dray|, the ray's largest S
        t = (np.sqrt(Sf) - np.abs(dray).astype(F)).astype(F)
        t_seg = np.stack([t[a:b].max(0) for a, b in cuts])
        e = (np.sqrt(S.max(0).astype(F)) * F(4.76837158203125e-7)).astype(F)
        v = F(0.5) * t_seg.max(0)
        lo, hi = (v - e).astype(F), (v + e).astype(F)
        hs = (F(0.5) * t_seg + e).astype(F)
    else:
        if plan.unit:  # fcm_pow_fold
            with np.errstate(divide="ignore", invalid="ignore"):
                r = (F(1.0) / np.sqrt(Sf)).astype(F)
                gm2 = np.where(S > 0, Sf * r, F(0.0)).astype(F)
                base = np.where(S > 0, F(1.0) - np.abs(dray).astype(F) * r, F(0.0)).astype(F)
            p, rel = _pow_fast(base, n)
            v = (F(0.5) * gm2 * p).astype(F)
            e = (v * (rel + F(4.76837158203125e-7)) + gm2 * (n * F(2.384185791015625e-7))).astype(F)
        else:          # fcm_value_fast: the reference's gradient in front of the fast power
            g = [(d.astype(F) / F(2.0)).astype(F) for d in (dzyx[2], dzyx[1], dzyx[0])]  # g0 = x, g1 = y, g2 = z
            gm = np.sqrt(((g[0] * g[0] + g[1] * g[1]).astype(F) + g[2] * g[2]).astype(F)).astype(F)
            d = g[2 - axis]
            with np.errstate(divide="ignore", invalid="ignore"):
                base = np.where(gm != 0, F(1.0) - np.abs(d / gm), F(0.0)).astype(F)
            p, rel = _pow_fast(base, n)
            v = np.moveaxis(np.where(gm != 0, gm * p, F(0.0)).astype(F), axis, 0)
            e = (v * np.moveaxis(rel, axis, 0)).astype(F)
        vlo, vhi = (v - e).astype(F), (v + e).astype(F)
        lo_seg = np.stack([vlo[a:b].max(0) for a, b in cuts])
        hs = np.stack([vhi[a:b].max(0) for a, b in cuts])
        lo, hi = lo_seg.max(0), hs.max(0)
    decided = (hi < F(32766.0)) & (np.trunc(lo).astype(np.int32) == np.trunc(hi).astype(np.int32))
    mask = np.zeros(lo.shape, np.uint32)
    for s in range(split):
        mask |= np.where(hs[s] >= lo, np.uint32(1) << np.uint32(s), np.uint32(0)).astype(np.uint32)
    mask = np.where(hi < F(32766.0), mask, np.uint32(0xFFFFFFFF))
    return Classified(~decided, np.where(decided, np.uint32(0), mask), lo, hi, plan)


# ================================================================================================================================
# volumes: rays laid along an axis
# ================================================================================================================================
def place(rays, axis):
    """rays[r, c, l] -> the dense volume whose ray (r, c) along `axis` is rays[r, c, :]; the picture is (nr, nc) for every axis"""
    order = {0: (2, 0, 1), 1: (0, 2, 1), 2: (0, 1, 2)}[axis]
    return np.ascontiguousarray(np.transpose(rays, order))


def as_axis0(rays):
    """the same rays as a (len, nr, nc) volume: what _slab_cases.lmip_walk / mida_walk read"""
    return place(rays, 0)


def grid_of(npix):
    """(nr, nc) with nr * nc == npix, more than one row wherever npix has a factor"""
    return {1: (1, 1), 63: (7, 9), 64: (4, 16), 65: (5, 13), 255: (15, 17), 256: (8, 32), 257: (1, 257), 128: (2, 64)}[npix]


STRIDED_LENS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49)
STRIDED_PIXELS = (63, 64, 65, 257)
STAGED_RAYS = (1, 63, 64, 65, 255, 256, 257)


def staged_lens(dtype):
    """CH - 1, CH, CH + 1, 2 CH, 2 CH + 1, a length whose byte length is no multiple of 16 (with a scalar tail of the LDS
    words for the types that can have one), and CH + one 16-byte vector: the 16-byte loads with a short last chunk"""
    ch = 128 // np.dtype(dtype).itemsize
    odd = {2: 2 * 64 + 7, 1: 128 + 13, 8: 16 + 5}[np.dtype(dtype).itemsize]
    return (ch - 1, ch, ch + 1, 2 * ch, 2 * ch + 1, odd, ch + 16 // np.dtype(dtype).itemsize)


# windows: (tmin, tmax) for LMIP, (wl, ww) for MIDA -- per dtype, on the value ranges of lmip_rays / mida_rays
LMIP_WINDOWS = {I16: ((0, 400), (-32768, 32767), (30000, 30100)), U8: ((10, 200), (0, 255), (254, 255)),
                F64: ((0.5, 400.25), (-1e300, 1e300), (30000.0, 30100.0))}
MIDA_WINDOWS = {I16: ((160, 80), (1600, 3000)), U8: ((100, 60), (128, 250)), F64: ((100, 60), (128, 250))}


def _seed(*parts):
    return sum((i + 1) * 7919 * int(p) for i, p in enumerate(parts)) % (2 ** 31)


def lmip_rays(npix, length, dtype, seed=0):
    """rays (nr, nc, len) for LMIP: each rises (with repeated values) to a peak at a depth drawn over the whole ray, falls by
    at least 1, and goes on with values on both sides of the peak -- a walk that reads on past its break, or stops a sample
    early, ends at another maximum.  One ray in eight never falls: its last sample is its maximum."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(_seed(npix, length, dtype.itemsize, seed, 1))
    nr, nc = grid_of(npix)
    small = dtype == U8
    rays = np.zeros((npix, length), np.int64)
    for i in range(npix):
        steps = (rng.random(length) < min(1.0, 40.0 / length)).astype(np.int64) if small else rng.integers(0, 12, length)
        rise = int(rng.integers(1, 12 if small else 60)) + np.cumsum(steps) - (0 if small else 40)
        peak = int(rng.integers(0, length))
        ray = rise.copy()
        if i % 8 != 7 and peak + 1 < length:
            ray[peak + 1] = rise[peak] - int(rng.integers(1, 3))
            ray[peak + 2:] = rise[peak] + rng.integers(-9 if small else -60, 10 if small else 300, max(0, length - peak - 2))
        rays[i] = ray
    if small:
        rays = np.clip(rays, 0, 255)
    out = rays.reshape(nr, nc, length)
    return (out * 0.75 + 0.125) if dtype == F64 else out.astype(dtype)


def mida_rays(npix, length, dtype, seed=0):
    """rays for MIDA_WINDOWS: noise below the narrow window with one sample above it at a depth drawn over the whole ray (the ray
    is opaque there: alpha goes from 0 to exactly 1) and brighter noise behind it, all of which lies on the wide window's ramp;
    one ray in four stays in the lowest fiftieth of the wide window's ramp all the way, so under that window every sample down
    to the last adds to its colour."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(_seed(npix, length, dtype.itemsize, seed, 2))
    nr, nc = grid_of(npix)
    small = dtype != I16
    lo_top, hi0, hi1 = (50, 150, 256) if small else (100, 220, 3000)
    rays = rng.integers(0, lo_top, (npix, length))
    for i in range(npix):
        if i % 4 == 3:
            rays[i] = rng.integers(4, 9, length) if small else rng.integers(100, 160, length)
            continue
        hit = int(rng.integers(0, length + 1))
        if hit < length:
            rays[i, hit] = int(rng.integers(hi0, hi1))
            rays[i, hit + 1:] = rng.integers(0, hi1, length - hit - 1)
    out = rays.reshape(nr, nc, length)
    return (out * 0.9 + 3.0) if dtype == F64 else out.astype(dtype)


# ---- early exit, built ---------------------------------------------------------------------------------------------------------
# A break AT sample k: sample k is the first below the running maximum with the window entered (LMIP: k >= 1, sample 0 is its
# own maximum), or the sample that takes alpha to 1 (MIDA: k >= 0).  -1: the ray is walked to its end.
def exit_depths(length):
    return (0, 1, 15, 16, length - 1)


def lmip_exit_ray(length, brk, rng):
    """int16 ray for the window (100, 5000): climbs inside the window, first falls at sample `brk` (0 stands for "the maximum is
    sample 0", which breaks at sample 1), then values above the old maximum that a walk going on would pick up"""
    if brk < 0:
        steps = rng.integers(0, 5, length)
        steps[-1] += 1  # (the last sample is the ray's only maximum)
        return 200 + np.cumsum(steps)
    brk = max(brk, 1)
    ray = np.empty(length, np.int64)
    ray[:brk] = 200 + np.cumsum(rng.integers(0, 5, brk))
    ray[brk] = ray[brk - 1] - 1
    ray[brk + 1:] = ray[brk - 1] + rng.integers(1, 900, length - brk - 1)
    return ray


def mida_exit_ray(length, brk, rng):
    """int16 ray for (wl, ww) = (1000, 200): below the window (alpha 0) up to sample `brk`, which lies above it (alpha 1); behind it
    samples in and above the window.  brk < 0: inside the lowest fiftieth of the ramp all the way: alpha stays far below 1."""
    if brk < 0:
        return rng.integers(900, 905, length)
    ray = rng.integers(0, 900, length)
    ray[brk] = 1101 + int(rng.integers(0, 2000))
    ray[brk + 1:] = rng.integers(900, 3200, length - brk - 1)
    return ray


EXIT_LMIP_WINDOW, EXIT_MIDA_WINDOW = (100, 5000), (1000, 200)
ExitCase = namedtuple("ExitCase", "name kind length rays breaks branch")


def _exit_case(kind, arrangement, length):
    """arrangement "wave": 128 rays, the first wave's 64 all break inside the first block (at 0, 1 and 15 in turn), the second
    wave's break at 16, at len - 1 or never; "alone": 64 rays break inside the first block except lane 37, which runs to the
    end of the ray"""
    rng = np.random.default_rng(_seed(length, len(arrangement), len(kind)))
    make = lmip_exit_ray if kind == "lmip" else mida_exit_ray
    if arrangement == "wave":
        breaks = [(0, 1, 15)[i % 3] for i in range(64)] + [(16, length - 1, -1)[i % 3] for i in range(64)]
        nr, nc = 2, 64
    else:
        breaks = [(0, 1, 15)[i % 3] for i in range(64)]
        breaks[37] = -1
        nr, nc = 1, 64
    rays = np.stack([make(length, b, rng) for b in breaks]).astype(np.int16).reshape(nr, nc, length)
    want = np.array(breaks).reshape(nr, nc)
    if kind == "lmip":
        want = np.where(want == 0, 1, want)
    return ExitCase("exit-%s-%s-len%d" % (kind, arrangement, length), kind, length, rays, want,
                    "exit-" + ("whole-wave-in-first-block" if arrangement == "wave" else "one-lane-runs-on"))


# 49: three blocks of the strided walk; 133: three chunks of the staged int16 walk (the first block / chunk holds samples 0..15 / 0..63)
EXIT_CASES = [_exit_case(k, a, n) for k in ("lmip", "mida") for a in ("wave", "alone") for n in (49, 133)]


# ================================================================================================================================
# the contour MaxIP
# ================================================================================================================================
def noise_volume(shape, seed):
    """int16 volume for the contour MaxIP: a quiet half (small differences: equal neighbours along the ray are common, so base 1
    and a zero gradient both occur), a loud half, a flat block, and the two ends of int16 next to each other (the T-subtraction
    wraps); its first and last rows and columns carry gradients like the rest"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-6, 7, shape).astype(np.int64)
    loud = rng.integers(-1500, 1500, shape)
    dz, dy, dx = shape
    z, y, x = np.indices(shape)
    v = np.where(2 * x >= dx, loud, v)
    v[: max(1, dz // 3), : max(1, dy // 3), : max(1, dx // 4)] = 17
    flat = v.reshape(-1)
    flat[:4] = [-32768, 32767, -32768, 32767]
    return v.astype(np.int16)


VARIANT_EXPONENTS = {1.0: 2, 0.5: 1, 2.0: 3, 3.3: 3, 100.0: 0, 0.0: 0}   # exponent -> FAST variant
VARIANT_SHAPES = ((75, 6, 16), (6, 75, 16), (7, 9, 72))                  # an axis-0 split, an axis-1 split, rows of 9 chunks

# depths: where the ray's maximum `value` lies; expect_bits: the segments k_fcm_max_decide must leave open; value_bits: those of
# them that hold the value (all of them unless stated)
FcmCase = namedtuple("FcmCase", "name vol axis n branch offset depths value expect_bits value_bits", defaults=(0, (), None, None, None))


def value_bits(case):
    return case.expect_bits if case.value_bits is None else case.value_bits


def h_profile(length, features):
    """h[l] with central difference h[l + 1] - h[l - 1] (ends clamped) equal to 0 exactly at the depths in `features` and 1 or 2
    everywhere else"""
    F_ = set(features)
    d = []
    for z in range(length - 1):
        if z in F_ or z + 1 in F_:
            d.append(0)
        elif z == 0 or z == length - 2 or z + 2 in F_:
            d.append(1)
        else:
            d.append(1 - d[-1])
    h = np.concatenate([[0], np.cumsum(d)]).astype(np.int64) if length > 1 else np.zeros(1, np.int64)
    k = np.arange(length)
    D = h[np.minimum(k + 1, length - 1)] - h[np.maximum(k - 1, 0)]
    assert set(np.flatnonzero(D == 0)) == F_ and D.max() <= 2, (length, features)
    return h


def ramp_volume(axis, length, a, b, features, nr, nc):
    """vol[l, r, c] = a r + b c + h[l] laid with l along `axis`: across the ray every interior voxel has the wrapped differences
    (2a, 2b); along it the difference is 0 at the depths in `features` and 1 or 2 elsewhere.  With a^2 + b^2 = c^2 an interior
    voxel's contour value is exactly c at a feature depth (gm = c, base = 1); where the difference along the ray is 1 it lies
    between c - 1 and c - 0.4 for the exponents 1 and 2 (a decoy), where it is 2 it is lower still.  features=None: h = 0, every depth is a feature (the plain ramp)."""
    h = np.zeros(length, np.int64) if features is None else h_profile(length, features)
    r, c = np.arange(nr)[:, None, None], np.arange(nc)[None, :, None]
    return place((a * r + b * c + h[None, None, :]).astype(np.int16), axis)


def flat_volume(axis, length, a, b, feature, decoy, decoy_d, nr, nc):
    """a flat background of zeros with two planes across the ray: the ramp a r + b c at depth `feature` (differences (2a, 2b, 0),
    value sqrt(a^2 + b^2)) and at depth `decoy` a plane whose differences are `decoy_d` = (Dr, Dc) (any integers: floor(D k / 2)
    has the central difference D everywhere), value sqrt(Dr^2 + Dc^2) / 2.  The planes next to each see only a difference along
    the ray: base 0."""
    r, c = np.arange(nr)[:, None], np.arange(nc)[None, :]
    rays = np.zeros((nr, nc, length), np.int64)
    rays[:, :, feature] = a * r + b * c
    rays[:, :, decoy] = (decoy_d[0] * r) // 2 + (decoy_d[1] * c) // 2
    assert abs(feature - decoy) >= 3 and np.abs(rays).max() < 32768
    return place(rays.astype(np.int16), axis)


# The decoy whose upper bound reaches the pixel's lower bound although it truncates one lower: the feature has the differences
# (0, 2000), value exactly 1000; the decoy (539, 1926): 539^2 + 1926^2 = 2000^2 - 3, value 999.999 625.  Either bound is at least
# 9.5e-4 away from the value at exponent 1 (the root of the ray's largest S, 2000 or more, times 2^-21) and 1.4e-3 at exponent 2: the
# decoy's upper bound passes the pixel's lower bound by four times the gap of 3.75e-4, which in turn is six float32 steps at 1000,
# so the reference's own rounding cannot close it (the host test asks the oracle).
LOWER_DECOY = (0, 1000, (539, 1926), 1000)   # a, b of the feature's ramp, the decoy's differences, the value


def interior(shape2):
    m = np.zeros(shape2, bool)
    m[1:-1, 1:-1] = True
    return m


TRIPLES = {0: (3, 4, 5), 1: (5, 12, 13), 2: (20, 21, 29)}   # per axis; (8, 15, 17) serves the flat-background cases


def _grid(axis):
    """(nr, nc) of the picture: one 8-voxel chunk along x for the rays across x; the rays along x are 64 voxels themselves"""
    return (4, 8) if axis != 2 else (5, 6)


def _segment_cases():
    """rays of 64, 75, 1 024 and 1 030 voxels along axes 0 and 1 on (len, 4, 8) and its twin: 2 segments of 32, 2 of 38 + 37, 32 of
    32, 31 of 33 and one of 7.  The ray's maximum in the first segment, in the last, on both sides of the first border, and where
    there are 32 segments on both sides of the last border and inside segment 31."""
    cases = []
    for axis in (0, 1):
        a, b, c = TRIPLES[axis]
        for length in (64, 75, 1024, 1030):
            for n in (1.0, 2.0):
                shape = place(np.zeros((4, 8, length), np.int16), axis).shape
                plan = fcm_plan(shape, axis, n)
                seg, split = plan.seg, plan.split
                spots = {"first-seg": 3, "last-seg": length - 3, "border-below": seg - 1, "border-above": seg}
                if split == 32:
                    spots.update({"last-border-below": 31 * seg - 1, "last-border-above": 31 * seg, "seg31": 31 * seg + plan.last_seg // 2})
                for tag, depth in spots.items():
                    cases.append(FcmCase("seg-ax%d-len%d-n%g-%s" % (axis, length, n, tag), ramp_volume(axis, length, a, b, (depth,), 4, 8),
                                         axis, n, "segments-len%d-%s" % (length, tag), 0, (depth,), c, (depth // seg,)))
    return cases


def _open_cases():
    cases = []
    for n in (1.0, 2.0):
        for axis in (0, 1, 2):
            a, b, c = TRIPLES[axis]
            nr, nc = _grid(axis)
            length = 64
            tag = "open-ax%d-n%g-" % (axis, n)
            seg = fcm_plan(place(np.zeros((nr, nc, length), np.int16), axis).shape, axis, n).seg
            # the feature behind the decoys of segment 0 (axis 2: one segment, the feature deep in the row)
            cases.append(FcmCase(tag + "feature-deep", ramp_volume(axis, length, a, b, (41,), nr, nc), axis, n, "open-feature-and-decoys",
                                 0, (41,), c, (41 // seg,)))
            # the mirror: two depths hold the value, in two segments where the ray splits -- two mask bits
            cases.append(FcmCase(tag + "mirror", ramp_volume(axis, length, a, b, (9, 50), nr, nc), axis, n, "open-mirror-two-bits",
                                 0, (9, 50), c, tuple(sorted({9 // seg, 50 // seg}))))
            # the plain ramp: every depth holds the value, every interior pixel is open with every segment
            split = cdiv(length, seg)
            cases.append(FcmCase(tag + "plain-ramp", ramp_volume(axis, length, a, b, None, nr, nc), axis, n, "open-every-interior-pixel",
                                 0, tuple(range(length)), c, tuple(range(split))))
            if axis != 2:  # (two segments) the mirror whose decoy truncates one lower, in front of the feature and behind it
                fa, fb, dd, val = LOWER_DECOY
                for where, feat, dec in (("front", 44, 12), ("behind", 12, 44)):
                    cases.append(FcmCase(tag + "mirror-lower-decoy-" + where, flat_volume(axis, length, fa, fb, feat, dec, dd, nr, nc), axis, n,
                                         "open-mirror-lower-decoy", 0, (feat,), val, (0, 1), (feat // seg,)))
            # flat background, one feature plane (8, 15, 17) and one decoy plane with differences (16, 29): 16.56, lower by 0.44
            cases.append(FcmCase(tag + "flat-background", flat_volume(axis, length, 8, 15, 44, 12, (16, 29), nr, nc), axis, n,
                                 "open-flat-background", 0, (44,), 17, (44 // seg,)))
    return cases


def _route_cases():
    cases = []
    for dx in (8, 16, 520, 61):
        shape = (6, 5, dx)
        vol = noise_volume(shape, 300 + dx)
        for axis in (0, 1, 2):
            for n in (1.0, 2.0):
                route = fcm_plan(shape, axis, n).route
                cases.append(FcmCase("route-dx%d-ax%d-n%g" % (dx, axis, n), vol, axis, n, "route-dx%d-%s" % (dx, route)))
    vol = noise_volume((6, 5, 16), 77)
    for axis in (0, 1, 2):
        for n in (1.0, 2.0):
            cases.append(FcmCase("route-unaligned-ax%d-n%g" % (axis, n), vol, axis, n, "route-unaligned-materialised", 2))
    return cases


def _variant_cases():
    cases = []
    for shape in VARIANT_SHAPES:
        vol = noise_volume(shape, 500 + shape[0])
        for n, fast in VARIANT_EXPONENTS.items():
            for axis in (0, 1, 2):
                kernel = "rows" if axis == 2 else "walk"
                cases.append(FcmCase("variant-%dx%dx%d-ax%d-n%g" % (shape + (axis, n)), vol, axis, n, "variant-FAST%d-%s" % (fast, kernel)))
    return cases


SEGMENT_CASES = _segment_cases()
OPEN_CASES = _open_cases()
FORCED_OPEN_CASES = OPEN_CASES + SEGMENT_CASES      # every one of them has interior pixels only k_fcm_fix can settle
ROUTE_CASES = _route_cases()
VARIANT_CASES = _variant_cases()
FCM_CASES = VARIANT_CASES + ROUTE_CASES + FORCED_OPEN_CASES
assert len({c.name for c in FCM_CASES}) == len(FCM_CASES)

# every branch of the contour MaxIP the edge tests are to reach; test_ray_cases_host.py proves each has a case
FCM_BRANCHES = (["variant-FAST%d-%s" % (f, k) for f in (0, 1, 2, 3) for k in ("walk", "rows")]
                + ["route-dx8-fused", "route-dx16-fused", "route-dx520-fused", "route-dx61-materialised", "route-unaligned-materialised"]
                + ["segments-len%d-%s" % (n, t) for n in (64, 75, 1024, 1030)
                   for t in ("first-seg", "last-seg", "border-below", "border-above")]
                + ["segments-len1024-seg31", "segments-len1030-seg31"]
                + ["open-feature-and-decoys", "open-mirror-two-bits", "open-every-interior-pixel", "open-flat-background", "open-mirror-lower-decoy"])


# ================================================================================================================================
# min / max
# ================================================================================================================================
def minmax_sizes(dtype):
    V = 16 // np.dtype(dtype).itemsize
    return sorted({1, V - 1, V, V + 1, 255, 256, 257, 2048 * 256 + 5} - {0})


MINMAX_ENDS = {I16: (-32768, 32767), U8: (0, 255), F64: (-98765.4321, 123456.789)}   # (neither double is a float32)


def minmax_base(n, dtype, seed=0):
    """values strictly between the two ends of MINMAX_ENDS"""
    rng = np.random.default_rng(_seed(n, np.dtype(dtype).itemsize, seed, 3))
    if np.dtype(dtype) == F64:
        return rng.uniform(-900.0, 900.0, n)
    return rng.integers(*((-900, 900) if np.dtype(dtype) == I16 else (40, 200)), n).astype(dtype)


def minmax_spots(n, dtype):
    """{name: element} where an extreme is put in turn: element 0, the vector body (its middle and its last element), the scalar
    tail (its first element) and the last element -- of the plan at an ALIGNED pointer; the same elements are used at the
    unaligned one, where everything is scalar"""
    p = minmax_plan(n, np.dtype(dtype).itemsize, 0)
    spots = {"first": 0, "last": n - 1}
    if p.body > 1:
        spots["body-middle"] = p.body // 2
        spots["body-end"] = p.body - 1
    if p.tail:
        spots["tail"] = p.body
    return spots


def ids(cases):
    return [c.name for c in cases]
