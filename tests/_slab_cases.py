"""Inputs for the Z-sharded step (invesalius3_amd/parallel.py, SlabVolume) and the thread runner that drives loop-back ranks
(tests/test_gpu_slab_edges.py on the GPU, tests/test_slab_cases_host.py anywhere).  Test infrastructure only: the product never
imports it.  Plain numpy / scipy.

A flood case is a boolean candidate volume (world * nz, dy, dx), global seeds (x, y, z) and a structuring element; the GPU tests
flood image_of(cand) between the thresholds (T0, T1).  The engine's constants a case is built around: a flood tile is 64 (x) x 16
(y) x 16 (z) voxels; rank r > 0 stores a bottom halo slice, so its top halo slice is local slice 1 + nz (nz for rank 0); a flood
that needs 48 rounds of tile visits is handed to the union-find engine.

    zigzag(world, nz, dy, dx, ncols, step)   one-voxel columns along z joined alternately at the top and the bottom of the
                                             volume: every column costs one exchange round per slab, every rank is resumed
                                             once per column and the vote is followed over a long run
    corner(world, nz, b, side, dx)           two voxels that touch by a corner only, across slab boundary b AND across a tile
                                             seam in y and x: the bit that arrives in the halo slice lies in another tile
                                             than the only voxel it can continue to
    corridor_above()                         a rank without a seed that needs hundreds of tile hops once a bit arrives
    blobs(world, nz, dy, dx, seed, empty)    smooth blobs at bone, optionally with one rank that holds no surface
    numpy_slabs(case)                        the case through parallel.slab_region_grow with the numpy backend: the reached
                                             set per rank and the number of exchange rounds (what the GPU is compared with)
    run_ranks(world, fn, device)             N ranks as threads over _ptr_comm.LoopbackWorld
    lmip_walk / mida_walk                    the Z rays of mips.rs in numpy, with the slice at which every ray breaks
"""
import functools
import threading
import traceback

import numpy as np
from scipy import ndimage

from _ptr_comm import LoopbackWorld

TX, TY, TZ = 64, 16, 16
ESCAPE = 48
IN, OUT, T0, T1 = 1000, -1000, 500, 3071
BONE = (226, 3071)
F = np.float32


def structure(conn):
    """conn 1 / 2 / 3 = 6 / 18 / 26 neighbours; "diag" = 6 neighbours and the pair (+1, +1, +1) / (-1, -1, -1): point-symmetric,
    none of scipy's three, so the engine takes its generic path (no coarse pass, k_flood_build_list)"""
    if conn == "diag":
        s = ndimage.generate_binary_structure(3, 1).copy()
        s[0, 0, 0] = s[2, 2, 2] = True
        return s
    return ndimage.generate_binary_structure(3, conn)


def image_of(cand):
    return np.where(cand, IN, OUT).astype(np.int16)


class Case:
    """cand (bool, z y x), seeds [(x, y, z)] in global coordinates, strct, and the sharding (world, nz) the case is built for"""

    def __init__(self, cand, seeds, strct, world, nz, img=None, **facts):
        assert cand.shape[0] == world * nz
        self.cand, self.seeds, self.strct, self.world, self.nz, self.img, self.facts = cand, list(seeds), strct, world, nz, img, facts
        cand.setflags(write=False)
        if img is not None:
            img.setflags(write=False)

    @property
    def shape(self):
        return self.cand.shape


def propagate(case):
    """the whole-volume reference: scipy's binary propagation of the in-candidate seeds inside cand"""
    seed = np.zeros(case.shape, bool)
    for x, y, z in case.seeds:
        seed[z, y, x] = case.cand[z, y, x]
    return ndimage.binary_propagation(seed, structure=case.strct, mask=case.cand)


# ---- flood cases -----------------------------------------------------------------------------------------------------------
ZIGZAG_ROUNDS = {(2, 16, 6): 8, (3, 15, 6): 14, (3, 16, 6): 14, (3, 17, 5): 12, (3, 33, 4): 10, (8, 2, 4): 30, (4, 1, 5): 8}
ZIGZAG_DY, ZIGZAG_STEP = 33, 25


@functools.lru_cache(maxsize=None)
def zigzag(world, nz, dy, dx, ncols, step, conn=1):
    """columns (y = dy // 2, x = k * step) over every slice; column k and k + 1 are joined by a run along x in the top slice
    for even k, in the bottom slice for odd k.  The seed is the foot of column 0."""
    dz, y = world * nz, dy // 2
    assert (ncols - 1) * step < dx and step >= 2
    cand = np.zeros((dz, dy, dx), bool)
    for k in range(ncols):
        cand[:, y, k * step] = True
        if k + 1 < ncols:
            cand[dz - 1 if k % 2 == 0 else 0, y, k * step:(k + 1) * step + 1] = True
    return Case(cand, [(0, y, 0)], structure(conn), world, nz, ncols=ncols)


CORNER_DY, CORNER_TAIL = 33, 30
CORNER_SHARDS = ((2, 16), (3, 15))


@functools.lru_cache(maxsize=None)
def corner(world, nz, b, side, dx, conn=3):
    """A = (z = b * nz - 1, y = 15, x = 63), the last slice of rank b - 1; B = (b * nz, 16, 64), the first slice of rank b.  A's
    tail runs to lower x in A's slice and then down in z, B's tail to higher x in B's slice and then up in z, both inside their
    own slab; no voxel of one side is a neighbour of a voxel of the other but A of B.  side "A" / "B": the seed is the far end
    of that tail."""
    assert 1 <= b < world and dx >= TX + 1 + CORNER_TAIL
    za, zb = b * nz - 1, b * nz
    up = min(nz - 1, 5)
    cand = np.zeros((world * nz, CORNER_DY, dx), bool)
    cand[za, 15, 63 - CORNER_TAIL + 1:64] = True
    cand[za - up:za + 1, 15, 63 - CORNER_TAIL + 1] = True
    cand[zb, 16, 64:64 + CORNER_TAIL] = True
    cand[zb:zb + up + 1, 16, 64 + CORNER_TAIL - 1] = True
    seed = (63 - CORNER_TAIL + 1, 15, za - up) if side == "A" else (64 + CORNER_TAIL - 1, 16, zb + up)
    half = int(cand[:zb].sum()), int(cand[zb:].sum())
    return Case(cand, [seed], structure(conn), world, nz, a=(za, 15, 63), b=(zb, 16, 64), side=side, half=half)


@functools.lru_cache(maxsize=None)
def corridor_above(conn=1):
    """world 2, nz 3: rank 1 holds _ccl_ref.serpentine() -- a voxel-wide corridor through 18 x 30 tiles of its middle slice --
    with (0, 0, 0) added, which joins the corridor's start to the column (y = 0, x = 0) that is all rank 0 holds"""
    from _ccl_ref import serpentine
    top = serpentine() == 1
    top[0, 0, 0] = True
    cand = np.zeros((6,) + top.shape[1:], bool)
    cand[:3, 0, 0] = True
    cand[3:] = top
    return Case(cand, [(0, 0, 0)], structure(conn), 2, 3, corridor=int(top[1].sum()))


# (world, nz, dy, dx, seed, empty_rank): the volumes of the repeated steps and of the stitch
STEP_BLOBS = [(3, 16, 48, 128, 11, None), (3, 16, 48, 80, 11, None)]
STITCH_BLOBS = [(3, 16, 40, 130, 12, None), (4, 2, 33, 128, 13, None), (8, 2, 20, 70, 16, None), (4, 15, 40, 128, 15, 1),
                (4, 15, 40, 128, 15, 3)]


@functools.lru_cache(maxsize=None)
def blobs(world, nz, dy, dx, seed, empty_rank=None):
    """conftest.synth_volume thresholded at bone; the seed is its brightest voxel, 26 neighbours.  With empty_rank that slab
    and the slices that touch it are below the threshold: its marching-cubes piece (its slices and the next one) has no
    surface.  case.img is the int16 volume itself."""
    from conftest import synth_volume
    img = synth_volume((world * nz, dy, dx), seed=seed)
    if empty_rank is not None:
        img[max(empty_rank * nz - 1, 0):(empty_rank + 1) * nz + 1] = -1024
    z, y, x = np.unravel_index(int(np.argmax(img)), img.shape)
    cand = (img >= BONE[0]) & (img <= BONE[1])
    return Case(cand, [(int(x), int(y), int(z))], structure(3), world, nz, img=img, empty_rank=empty_rank)


# ---- ranks as threads --------------------------------------------------------------------------------------------------------
def run_ranks(world, fn, device=True, timeout=300):
    """fn(rank, comm) on `world` threads over one LoopbackWorld; returns (the world, [fn's result per rank]).  A rank that raises
    breaks the others' barrier, and its traceback is the failure."""
    lw = LoopbackWorld(world, device=device)
    res, errs = {}, []

    def run(rank):
        try:
            res[rank] = fn(rank, lw.comm(rank))
        except Exception:  # pragma: no cover
            errs.append((rank, traceback.format_exc()))
            lw.barrier.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=timeout) for t in th]
    assert not errs, "\n".join("rank %d: %s" % e for e in errs)
    assert not any(t.is_alive() for t in th), "a rank did not finish"
    return lw, [res[r] for r in range(world)]


@functools.lru_cache(maxsize=None)
def numpy_slabs(case):
    """The case through parallel.slab_region_grow with _gloo_worker.NumpyBackend on host pointers, one thread per rank.
    Returns (exchange rounds, [per rank: dict(lay, reached (stored slices, halo included), nseeds, reads)])."""
    from _gloo_worker import NumpyBackend
    from invesalius3_amd import parallel as par

    def rank_fn(rank, comm):
        lay = par.slab_layout(rank, case.world, case.nz)
        lo = lay.z_global0 - lay.hb
        cand = case.cand[lo:lo + lay.local_dz].copy()
        reached = np.zeros_like(cand)
        loc = par.local_seeds(lay, case.seeds)
        for x, y, z in loc:
            reached[z, y, x] = cand[z, y, x]
        be = NumpyBackend(cand, reached, case.strct, lay)
        rounds = par.slab_region_grow(be, comm, lay)
        return dict(lay=lay, reached=be.reached, nseeds=len(loc), reads=be.reads, rounds=rounds)

    _, res = run_ranks(case.world, rank_fn, device=False)
    rounds = {r["rounds"] for r in res}
    assert len(rounds) == 1 and all(r["reads"] == r["rounds"] for r in res)
    return rounds.pop(), res


# ---- bit planes --------------------------------------------------------------------------------------------------------------
def pack_plane(bits):
    """(..., dx) bool -> (..., ceil(dx / 64)) uint64: bit x & 63 of word x / 64 (the layout of the engine's planes; the bits
    beyond dx in a ragged last word are 0).  For dx % 64 == 0 the bytes are those of _plane() in test_gpu_flood_apply_levels.py."""
    bits = np.asarray(bits, bool)
    wx = -(-bits.shape[-1] // 64)
    pad = np.zeros(bits.shape[:-1] + (wx * 64,), bool)
    pad[..., :bits.shape[-1]] = bits
    return np.packbits(pad.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint64).reshape(bits.shape[:-1] + (wx,))


def unpack_plane(words, dx=None):
    """(..., wx) uint64 -> (..., wx * 64) bool, cut to dx when given"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    bits = np.unpackbits(words.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little").reshape(words.shape[:-1] + (-1,)).astype(bool)
    return bits if dx is None else bits[..., :dx]


# ---- Z rays with their break index ---------------------------------------------------------------------------------------------
RAY_SHAPE, RAY_SEED = (70, 5, 67), 91
RAY_CUTS = ([1, 16, 17, 33, 65], [15, 31], [32], [33, 66], [1, 2, 3])


def pieces(dz, cuts):
    edges = [0] + list(cuts) + [dz]
    return list(zip(edges[:-1], edges[1:]))


def lmip_walk(img, tmin, tmax):
    """lmip of mips.rs:7-86 along axis 0 as tests/test_oracle_mips.py states it; returns (image, break index per ray, -1 for
    a ray that is walked to its end)"""
    dz, dy, dx = img.shape
    out = np.zeros((dy, dx), img.dtype)
    brk = np.full((dy, dx), -1, np.int64)
    for y in range(dy):
        for x in range(dx):
            ray = img[:, y, x].tolist()
            max_val = ray[0]
            start = tmin <= max_val <= tmax
            for i, val in enumerate(ray):
                if val > max_val:
                    max_val = val
                elif val < max_val and start:
                    brk[y, x] = i
                    break
                if tmin <= val <= tmax:
                    start = True
            out[y, x] = max_val
    return out, brk


def mida_walk(img, wl, ww):
    """mida_internal of mips.rs:88-168 along axis 0 for an int16 volume, every ray at once in float32 arrays (one rounding per
    operation, the reference's order); returns (image, break index per ray, -1 for a ray whose alpha never reaches 1)"""
    f = img.astype(F)
    img_min, img_max = F(f.min()), F(f.max())
    rng = F(img_max - img_min)
    inv = F(F(1.0) / rng)
    lo, hi = F(F(wl) - F(F(ww) / F(2.0))), F(F(wl) + F(F(ww) / F(2.0)))
    shp = img.shape[1:]
    fmax, alpha_p, colour_p, final = (np.zeros(shp, F) for _ in range(4))
    brk = np.full(shp, -1, np.int64)
    live = np.ones(shp, bool)
    one = F(1.0)
    for i in range(img.shape[0]):
        vl = f[i]
        fpi = inv * (vl - img_min)
        gt = fpi > fmax
        dl = np.where(gt, fpi - fmax, F(0.0)).astype(F)
        bt = one - dl
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = np.where(vl < lo, F(0.0), np.where(vl > hi, one, (vl - lo) / F(hi - lo))).astype(F)
        rest = one - bt * alpha_p
        colour = bt * colour_p + (rest * fpi) * alpha
        cur = bt * alpha_p + rest * alpha
        assert colour.dtype == F and cur.dtype == F
        fmax = np.where(live & gt, fpi, fmax)
        colour_p = np.where(live, colour, colour_p)
        alpha_p = np.where(live, cur, alpha_p)
        final = np.where(live, colour, final)
        ends = live & (cur >= one)
        brk[ends] = i
        live &= ~ends
    v = rng * final + img_min
    assert (v > F(-32769.0)).all() and (v < F(32768.0)).all()
    return np.trunc(v).astype(np.int16), brk
