"""Inputs for the wake-up rule of the region-growing rounds (csrc/k_flood.hip, tile_update): after a visit a neighbour tile is
woken only when the visit's staged halo holds a voxel of that tile that was unreached, lies in the 3 x 3 x 3 neighbourhood of one
of the visit's new bits and (but for the voxels beside the tile's words) is a candidate (tests/test_gpu_flood_wake.py on the GPU, tests/test_flood_wake_cases_host.py
anywhere).  Test infrastructure only: the product never imports it.  Plain numpy / scipy.

    contacts_case(shape, centre)   (a), (e), (f) a body in one tile that touches ONE candidate voxel of each neighbour tile
    stale_halo_case()              (b) two seeded bodies in neighbouring tiles and parts only reachable through the other tile
    no_wake_case(axis)             (c) a line of tiles whose bodies end one empty row short of each other
    chain_case()                   (d) a voxel-wide snake through nine tiles, one tile per round
    propagate_flood(...)           the flood of any 3 x 3 x 3 structuring element (asymmetric ones too) by propagation
    model_rounds(...)              numpy restatement of the rounds: visits, rounds, first list for the rules "open" and "faces"
"""
import functools

import numpy as np
from scipy import ndimage

import _flood_cases as fc
from _flood_cases import T0, T1, TX, TY, TZ, VAL, Case, label_flood  # noqa: F401  (re-exported for the tests)

ITCAP = 24  # flood_tiles.h: local iterations per visit
SHAPE = (48, 48, 192)  # 3 x 3 x 3 tiles


def asym_structure():
    """a 3 x 3 x 3 structuring element that is not point-symmetric (the engine's generic path): all 26 neighbours but the
    steps (+1, +1, +1) and (-1, 0, 0) in (z, y, x)"""
    s = np.ones((3, 3, 3), bool)
    s[2, 2, 2] = False
    s[0, 1, 1] = False
    return s


def propagate_flood(img, seeds, fill, strct, out):
    """floodfill_threshold for any structuring element: reached voxel p reaches p + k for every set offset k of `strct`
    (a Minkowski sum, scipy's binary dilation), inside the candidates (in range, out != fill; in-range seeds always)"""
    inr = (img >= T0) & (img <= T1)
    c = inr & (out != fill)
    r = np.zeros(img.shape, bool)
    for x, y, z in seeds:
        if inr[z, y, x]:
            c[z, y, x] = r[z, y, x] = True
    s = np.asarray(strct, bool).copy()
    s[1, 1, 1] = True
    out[ndimage.binary_propagation(r, structure=s, mask=c)] = fill


# ---- (a), (e), (f): one contact per direction -----------------------------------------------------------------------------
DIRS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dz or dy or dx]


@functools.lru_cache(maxsize=None)
def contacts_case(shape=SHAPE, centre=(1, 1, 1)):
    """The tile `centre` (tz, ty, tx) is a body but for one missing voxel in each of its 16-voxel blocks (no block is
    all-candidate: the rounds flood it, not the coarse pass); the seed is inside it.  For every direction d whose voxels exist
    in `shape`, the neighbour tile in direction d holds ONE candidate next to the body -- beside the middle of the face, the
    edge, or the corner voxel, so a pure +-x contact is bit 63 / bit 0 of the neighbour word -- and a tail of three more
    voxels behind it, along the first axis d moves on, away from the body.  Contacts and tails of different directions are at
    least eight voxels apart.  facts: contacts = {d: (contact voxel, tail voxels)} in (z, y, x)."""
    dz, dy, dx = shape
    cz, cy, cx = centre
    lo = (cz * TZ, cy * TY, cx * TX)
    hi = (min(lo[0] + TZ, dz) - 1, min(lo[1] + TY, dy) - 1, min(lo[2] + TX, dx) - 1)
    assert hi == (lo[0] + TZ - 1, lo[1] + TY - 1, lo[2] + TX - 1), "the centre tile is a whole tile"
    img = np.zeros(shape, np.int16)
    img[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = VAL
    for k in range(TX // 16):
        img[lo[0] + 4, lo[1] + 4, lo[2] + 8 + 16 * k] = 0
    mid = (lo[0] + 8, lo[1] + 8, lo[2] + 32)
    contacts = {}
    for d in DIRS:
        v = tuple(lo[a] - 1 if d[a] < 0 else hi[a] + 1 if d[a] > 0 else mid[a] for a in range(3))
        ax = next(a for a in range(3) if d[a])
        tail = [tuple(v[a] + (k * d[a] if a == ax else 0) for a in range(3)) for k in (1, 2, 3)]
        if all(0 <= p[a] < shape[a] for p in [v] + tail for a in range(3)):
            contacts[d] = (v, tail)
            for p in [v] + tail:
                img[p] = VAL
    seed = (lo[2] + 6, lo[1] + 10, lo[0] + 10)  # (x, y, z)
    return Case(img, np.zeros(shape, np.uint8), [("body", [seed], 1)], contacts=contacts, lo=lo, hi=hi)


def contacts_reached(case, strct):
    """{d: the contact voxel of direction d connects under `strct`}: the body's voxel(s) it touches reach it by a set offset"""
    s = np.asarray(strct, bool)
    lo, hi = case.facts["lo"], case.facts["hi"]
    res = {}
    for d, (v, _) in case.facts["contacts"].items():
        ok = False
        for k in DIRS:  # u = v - k in the body, step k set
            u = tuple(v[a] - k[a] for a in range(3))
            if s[k[0] + 1, k[1] + 1, k[2] + 1] and all(lo[a] <= u[a] <= hi[a] for a in range(3)) and case.img[u] == VAL:
                ok = True
        res[d] = ok
    return res


# ---- (b): a stale halo --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stale_halo_case():
    """Tiles A = (1, 0, 1) and B = (1, 1, 1) share the face y = 15 | 16.  A1 (seeded) and B1 (seeded) both reach it and touch;
    A2 is joined to the rest through B1 only, B2 through A2 only: whichever of A and B stages its halo first in the first
    round, the other must be woken for what it could not see yet, twice over."""
    img = np.zeros(SHAPE, np.int16)
    bodies = {"A1": (slice(17, 20), slice(4, 16), slice(70, 91)), "B1": (slice(17, 24), slice(16, 29), slice(70, 91)),
              "A2": (slice(22, 27), slice(4, 16), slice(70, 91)), "B2": (slice(26, 30), slice(16, 29), slice(70, 91))}
    for v in bodies.values():
        img[v] = VAL
    return Case(img, np.zeros(SHAPE, np.uint8), [("both", [(80, 6, 18), (80, 26, 22)], 1)], bodies=bodies)


# ---- (c): wake-ups that must not happen ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def no_wake_case(axis):
    """axis 1 (y) or 0 (z): the three tiles of the middle line along that axis each hold a body that starts on the tile's
    second row (slice) and fills its face towards the next tile, so the next tile has no candidate within one voxel of that
    face.  The seed is in the middle tile's body: it floods in one visit and changes the whole face, and nothing of the
    next tile is next to it.  Along x and the other axis the bodies stay two voxels inside the tile."""
    img = np.zeros(SHAPE, np.int16)
    for k in range(3):
        box = [slice(18, 30), slice(18, 30), slice(66, 126)]
        box[axis] = slice(16 * k + 1, 16 * k + 16)
        img[tuple(box)] = VAL
    seed = (96, 24, 24)
    return Case(img, np.zeros(SHAPE, np.uint8), [("middle", [seed], 1)])


# ---- (d): a single chain -----------------------------------------------------------------------------------------------------
CHAIN = [(1, 0, 0), (1, 0, 1), (1, 0, 2), (1, 1, 2), (1, 1, 1), (1, 1, 0), (1, 2, 0), (1, 2, 1), (1, 2, 2)]  # (tz, ty, tx)


@functools.lru_cache(maxsize=None)
def chain_case():
    """A voxel-wide snake in the slice z = 24 through the nine tiles of CHAIN: down x = 5 from the seed at y = 1 to y = 14
    (thirteen local iterations: the seeded tile publishes long after the other tiles of the first list have staged their
    halos, so the first round is as deterministic as the later ones), along y = 14 to x = 180, down to y = 30, back to
    x = 5, down to y = 46, along y = 46 to x = 180.  A horizontal stretch fills in one iteration (run closure), a vertical
    one takes at most 16 < ITCAP, and the snake keeps five voxels away from every tile corner: each visit has exactly one
    open candidate in its halo, the next tile's, so every round after the first has a list of one tile."""
    img = np.zeros(SHAPE, np.int16)
    z = 24
    img[z, 1:15, 5] = VAL
    img[z, 14, 5:181] = VAL
    img[z, 14:31, 180] = VAL
    img[z, 30, 5:181] = VAL
    img[z, 30:47, 5] = VAL
    img[z, 46, 5:181] = VAL
    return Case(img, np.zeros(SHAPE, np.uint8), [("snake", [(5, 1, z)], 1)], tiles=len(CHAIN))


# ---- the rounds, restated ------------------------------------------------------------------------------------------------------
def _close_runs(r, c):
    """every candidate run along x that holds a reached voxel becomes reached"""
    while True:
        n = r.copy()
        n[..., 1:] |= r[..., :-1] & c[..., 1:]
        n[..., :-1] |= r[..., 1:] & c[..., :-1]
        if (n == r).all():
            return r
        r = n


def model_rounds(img, seeds, rule="open", itcap=ITCAP):
    """The rounds of a 26-neighbour flood with the fused start, every tile of a round's list staged from the same snapshot:
    (rounds that had a list, visits, length of the first list, reached).  The first list is the 3 x 3 x 3 tile
    neighbourhood of the seeds' tiles (no tile of these cases is wholly reached by the coarse pass).  A visit: at most
    `itcap` iterations of "OR of the 26 neighbours AND candidates, close the x-runs" on the tile with a one-voxel halo
    that stays as staged; it wakes itself when the cap ended it, and its neighbour tiles by `rule`: "faces" = every tile
    that can see a changed face, edge or corner; "open" (the kernel's) = only for a staged halo voxel of that tile that
    was unreached, lies in the 3 x 3 x 3 neighbourhood of a new bit and -- in the halo rows above, below, before and behind
    the tile; the voxels beside the tile's words are not asked -- is a candidate.  A tile that a visit leaves without an
    unreached candidate is closed and never woken again."""
    dz, dy, dx = img.shape
    assert dz % TZ == 0 and dy % TY == 0 and dx % TX == 0
    ntz, nty, ntx = dz // TZ, dy // TY, dx // TX
    c = (img >= T0) & (img <= T1)
    r = np.zeros(img.shape, bool)
    cur = set()
    for x, y, z in seeds:
        r[z, y, x] = True
        for a in DIRS + [(0, 0, 0)]:
            t = (z // TZ + a[0], y // TY + a[1], x // TX + a[2])
            if 0 <= t[0] < ntz and 0 <= t[1] < nty and 0 <= t[2] < ntx:
                cur.add(t)
    first, rounds, visits = len(cur), 0, 0
    closed = set()
    s26 = np.ones((3, 3, 3), bool)
    sl = {-1: slice(0, 1), 0: slice(1, -1), 1: slice(-1, None)}
    while cur:
        rounds += 1
        visits += len(cur)
        rp, cp = np.pad(r, 1), np.pad(c, 1)
        nxt = set()
        for tz, ty, tx in sorted(cur):
            win = (slice(tz * TZ, tz * TZ + TZ + 2), slice(ty * TY, ty * TY + TY + 2), slice(tx * TX, tx * TX + TX + 2))
            rw, cw = rp[win].copy(), cp[win]
            r_in = rw[1:-1, 1:-1, 1:-1].copy()
            exhausted = True
            for _ in range(itcap):
                n = rw[1:-1, 1:-1, 1:-1] | (ndimage.binary_dilation(rw, structure=s26)[1:-1, 1:-1, 1:-1] & cw[1:-1, 1:-1, 1:-1])
                n = _close_runs(n, cw[1:-1, 1:-1, 1:-1])
                if (n == rw[1:-1, 1:-1, 1:-1]).all():
                    exhausted = False
                    break
                rw[1:-1, 1:-1, 1:-1] = n
            chg = rw[1:-1, 1:-1, 1:-1] & ~r_in
            if not (cw[1:-1, 1:-1, 1:-1] & ~rw[1:-1, 1:-1, 1:-1]).any():
                closed.add((tz, ty, tx))
            if not chg.any():
                continue
            r[tz * TZ:(tz + 1) * TZ, ty * TY:(ty + 1) * TY, tx * TX:(tx + 1) * TX] |= chg
            if exhausted:
                nxt.add((tz, ty, tx))
            near = ndimage.binary_dilation(np.pad(chg, 1), structure=s26)
            if rule == "open":
                front = near & ~rp[win]
                front[:, :, 1:-1] &= cw[:, :, 1:-1]
            else:
                front = near
            front[1:-1, 1:-1, 1:-1] = False
            for d in DIRS:
                t = (tz + d[0], ty + d[1], tx + d[2])
                if 0 <= t[0] < ntz and 0 <= t[1] < nty and 0 <= t[2] < ntx and front[sl[d[0]], sl[d[1]], sl[d[2]]].any():
                    nxt.add(t)
        cur = nxt - closed
    return rounds, visits, first, r
