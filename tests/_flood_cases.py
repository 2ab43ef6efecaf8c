"""Inputs for the coarse pass of the region-growing engine (csrc/k_flood.hip): k_flood_block_flags -> k_flood_coarse ->
k_flood_block_apply, and the size limits around it (tests/test_gpu_flood_coarse.py on the GPU,
tests/test_flood_cases_host.py anywhere).  Test infrastructure only: the product never imports it.  Plain numpy / scipy.

The engine's constants, restated here so that a case can say which path it is built for (the host test holds them against
ivx_flood_describe, i.e. against the engine's own decisions):
    tile = 64 (x) x 16 (y) x 16 (z) voxels; a row of tiles along x is one 64-bit word of block bits
    block width 16 up to 1024 voxels along x, 32 up to 2048, 64 up to 4096; beyond that the pass is off
    the coarse workgroup has 64..1024 lanes (the power of two >= rows), then up to 8 rows per lane
    the pass is off at (nty + 2) * (ntz + 2) > 7680 or nty * ntz > 8192
    <= 16 seeds ride on the coarse pass (fused start); a round is launched with at most 1536 workgroups;
    seeds are staged 4096 at a time; the counter ring holds 16 rounds; past 48 rounds the union-find engine takes over

    widths_case(dx)      (a) bodies on the block grid of that width, their contacts, the four floods of the run-through
    rows_case(name)      (c) thin volumes with 65 / 1025 / 86 x 85 / 86 x 86 rows of tiles
    tile_serpentine()    (d) corridors of whole tiles, more than 48 tile hops long
    all_candidate(dx)    (d) nothing but candidates, one per block width
    long_list()          (e) noise with 5000 seeds: a first round of more than 1536 tiles, two staging chunks
    ring_corridor()      (e) a voxel-wide corridor of 30 tiles: 17..47 rounds
    run_floods(case, conn, flood)   the floods of a case through `flood` (the oracle's or the product's floodfill_threshold)
    label_floods(case, conn)        the same from scipy.ndimage.label: "the labelled components that hold an in-range seed"
"""
import functools

import numpy as np
from scipy import ndimage

TX, TY, TZ = 64, 16, 16
VAL, T0, T1 = 500, 400, 600
CROWS_MAX, CT, CRP = 7680, 1024, 8
GRID_CAP, FUSED_SEEDS, SEED_CHUNK, RING, ESCAPE = 1536, 16, 4096, 16, 48


def structure(conn):
    """conn 1 / 2 / 3 = 6 / 18 / 26 neighbours"""
    return ndimage.generate_binary_structure(3, conn)


# ---- the engine's path, from its constants -------------------------------------------------------------------------------
def block_width(dx):
    wx = -(-dx // TX)
    return 16 if wx <= 16 else 32 if wx <= 32 else 64 if wx <= 64 else 0


def expected_path(shape, nseeds):
    """what ivx_flood_describe must return for a standard structuring element and no IVX_FLOOD_* switch"""
    dz, dy, dx = shape
    wx, nty, ntz = -(-dx // TX), -(-dy // TY), -(-dz // TZ)
    rows = nty * ntz
    on = wx <= 64 and (nty + 2) * (ntz + 2) <= CROWS_MAX and rows <= CT * CRP
    lanes = 64
    while lanes < CT and lanes < rows:
        lanes *= 2
    bxs = block_width(dx)
    ntiles = wx * rows
    return [int(on), bxs if on else 0, TX // bxs if on else 0, lanes if on else 0, -(-rows // lanes) if on else 0,
            int(on and 1 <= nseeds <= FUSED_SEEDS), min(ntiles, GRID_CAP), ntiles]


class Case:
    """img (int16, z y x), out0 (uint8: the pre-filled out array) and floods = [(name, seeds (x, y, z), fill)], run one
    after the other into the same out array when `chained`, else each into a copy of out0.  bodies = {name: box slices};
    joined[conn][flood name] = the bodies that flood fills (a construction fact, held against both references on the CPU)."""

    def __init__(self, img, out0, floods, chained=(), bodies=None, joined=None, **facts):
        self.img, self.out0, self.floods, self.chained = img, out0, floods, set(chained)
        self.bodies, self.joined = bodies or {}, joined or {}
        self.facts = facts
        img.setflags(write=False)
        out0.setflags(write=False)

    @property
    def shape(self):
        return self.img.shape


def run_floods(case, conn, flood):
    """[(name, fill, out before, out after)] of the case's floods through flood(img, seeds, t0, t1, fill, strct, out)"""
    res, prev = [], None
    for name, seeds, fill in case.floods:
        before = prev.copy() if (name in case.chained and prev is not None) else case.out0.copy()
        after = before.copy()
        flood(case.img, seeds, T0, T1, fill, structure(conn), after)
        res.append((name, fill, before, after))
        prev = after
    return res


def label_flood(img, seeds, fill, conn, out):
    """floodfill_threshold by labelling: the components of (t0 <= img <= t1) & (out != fill) that hold a seed, plus the
    in-range seeds themselves (a seed on a pre-filled voxel is still filled; its neighbours are reached from it)"""
    inr = (img >= T0) & (img <= T1)
    c = inr & (out != fill)
    for x, y, z in seeds:
        if inr[z, y, x]:
            c[z, y, x] = True
    lab, _ = ndimage.label(c, structure=structure(conn))
    ids = {int(lab[z, y, x]) for x, y, z in seeds if inr[z, y, x]}
    ids.discard(0)
    out[np.isin(lab, sorted(ids))] = fill


def label_floods(case, conn):
    return run_floods(case, conn, lambda img, seeds, t0, t1, fill, strct, out: label_flood(img, seeds, fill, conn, out))


def loose_voxels(shape, bodies_mask, keep_out, density, seed, body_ids=None):
    """Random candidate voxels around the bodies that can never change which bodies join: no voxel inside `keep_out`
    (the gaps that must stay empty), and every 26-connected cluster of loose voxels that touches two different bodies is
    dropped whole (26 contains 6 and 18, so what cannot bridge under 26 cannot bridge at all)."""
    rng = np.random.default_rng(seed)
    loose = (rng.random(shape) < density) & ~bodies_mask & ~keep_out
    if body_ids is None:
        return loose
    s26 = structure(3)
    lab, n = ndimage.label(loose, structure=s26)
    touch = np.zeros((n + 1, int(body_ids.max()) + 1), bool)
    for b, box in enumerate(ndimage.find_objects(body_ids), 1):  # bodies are boxes: look one voxel around each
        if box is None:
            continue
        win = tuple(slice(max(v.start - 1, 0), v.stop + 1) for v in box)
        near = ndimage.binary_dilation(body_ids[win] == b, structure=s26) & loose[win]
        touch[np.unique(lab[win][near]), b] = True
    bad = touch.sum(1) >= 2
    bad[0] = False
    return loose & ~bad[lab]


def whole_block_share(case, fill):
    """(all-candidate blocks, existing blocks) of the case's first candidate plane for `fill`, blocks of the engine's width"""
    dz, dy, dx = case.shape
    b = block_width(dx) or 64
    c = (case.img >= T0) & (case.img <= T1) & (case.out0 != fill)
    nz, ny, nx = -(-dz // TZ), -(-dy // TY), -(-dx // b)
    pad = np.ones((nz * TZ, ny * TY, nx * b), bool)  # out-of-bounds voxels do not count against a block
    pad[:dz, :dy, :dx] = c
    whole = pad.reshape(nz, TZ, ny, TY, nx, b).all(axis=(1, 3, 5))
    return int(whole.sum()), nz * ny * nx


# ---- (a) block widths -----------------------------------------------------------------------------------------------------
WIDTHS = (1024, 1025, 1100, 2048, 2049, 2500, 4096, 4097)
DZ_A, DY_A = 18, 35  # two tile slices (16 + 2) and three tile rows (16 + 16 + 3): partial tiles on the high sides
Z0, Z1, ZALL = slice(0, 16), slice(16, 18), slice(0, 18)
Y0, Y1, Y2 = slice(0, 16), slice(16, 32), slice(32, 35)
BODY_NAMES = ("A", "B", "C", "D", "E", "F", "G", "H", "G2", "H2", "T", "L")


@functools.lru_cache(maxsize=None)
def widths_case(dx):
    """Boxes on the block grid of this width (b = block width; beyond 4096 voxels, where the pass is off, b = 64):
      B | A    face neighbours across the word boundary x = 128, rows (Z0, Y1)
      C        (Z0, Y0), starts where A ends (x = 256 + b % 64: a block boundary inside a word when b < 64): an edge of A only
      D        (Z1, Y2), same x as C: a corner of A only (and two tile rows away from C)
      E        (Z0, Y1), ends one voxel short of the block boundary x = 448 + b: its last block is not whole
      F        (Z0, Y0), the one block beside E's last, short one: joins E by a face, whatever the structure
      G . H    (all z, Y0), one empty block between them;   G2 . H2  (all z, Y2), one empty voxel plane between them
      T        (Z0, Y1), two whole tiles, one whole block and half a block (the tail), alone in a zone without loose voxels
               that reaches one tile beyond it on either side: the tail shares its tile with a wholly reached block, no
               visit of a neighbour tile ever changes a face it could see, and its seed is two tiles away -- only
               k_flood_block_apply's own enlisting of that tile gets the tail filled
      L        (all z, Y1), from one block before the last word to dx - 1
    out0: a slab of 1s inside E (barriers of the floods with fill 1) and a slab of 2s inside A (barriers of the flood with
    fill 2 only: blocks that were whole in the first floods are partly blocked in the last one).
    Floods: one seed in a whole block of A; one seed in E's last block (a tile that is not whole); 17 seeds (the unfused
    start: A, E, G, G2, T, L, six loose voxels, five voxels out of range); then, into the out array the 17 seeds left, a
    flood with fill 2 from A, H, H2 and T."""
    b = block_width(dx) or 64
    shape = (DZ_A, DY_A, dx)
    a1 = 256 + b % 64
    e1 = 448 + b
    l0 = TX * (-(-dx // TX) - 1) - b
    t0x = -(-(576 + 4 * b) // TX) * TX + TX
    t1x = t0x + 2 * TX + b + b // 2
    bodies = {
        "B": (Z0, Y1, slice(64, 128)), "A": (Z0, Y1, slice(128, a1)),
        "C": (Z0, Y0, slice(a1, a1 + b)), "D": (Z1, Y2, slice(a1, a1 + b)),
        "E": (Z0, Y1, slice(384, e1 - 1)), "F": (Z0, Y0, slice(e1 - b, e1)),
        "G": (ZALL, Y0, slice(576, 576 + 2 * b)), "H": (ZALL, Y0, slice(576 + 3 * b, 576 + 4 * b)),
        "G2": (ZALL, Y2, slice(576, 576 + 2 * b)), "H2": (ZALL, Y2, slice(576 + 2 * b + 1, 576 + 4 * b)),
        "T": (Z0, Y1, slice(t0x, t1x)), "L": (ZALL, Y1, slice(l0, dx)),
    }
    assert 576 + 4 * b <= t0x - TX and t1x < l0 - b
    img = np.zeros(shape, np.int16)
    ids = np.zeros(shape, np.int8)
    for n, name in enumerate(BODY_NAMES, 1):
        assert not ids[bodies[name]].any()
        img[bodies[name]] = VAL
        ids[bodies[name]] = n
    keep_out = np.zeros(shape, bool)
    keep_out[:, :, 576 + 2 * b:576 + 3 * b] = True   # the empty block between G and H (and the plane between G2 and H2)
    keep_out[:, :, e1 - 1] = True                     # the plane E stops short of
    keep_out[:, :, t0x - TX:-(-t1x // TX) * TX + TX] = True  # T's zone
    out0 = np.zeros(shape, np.uint8)
    out0[4:8, 20:28, 400:410] = 1                     # inside E
    out0[2:6, 18:30, 140:150] = 2                     # inside A
    loose = loose_voxels(shape, ids > 0, keep_out, 0.03, 1000 + dx, ids)
    img[loose] = VAL
    rng = np.random.default_rng(2000 + dx)
    li = np.argwhere(loose)
    li = li[rng.choice(len(li), 6, replace=False)]
    ei = np.argwhere(img == 0)
    ei = ei[rng.choice(len(ei), 5, replace=False)]
    s_a, s_a2 = (128 + b + 3, 20, 5), (a1 - 3, 25, 12)  # s_a2: A's last block, clear of the slab of 2s
    s_e = (e1 - 3, 20, 5)
    s_t = (t0x + 5, 22, 9)
    many = [s_a, s_e, (576 + 3, 5, 17), (576 + b + 2, 33, 3), s_t, (dx - 1, 30, 16)]
    many += [(int(x), int(y), int(z)) for z, y, x in li] + [(int(x), int(y), int(z)) for z, y, x in ei]
    floods = [("one_in_A", [s_a], 1), ("one_in_E", [s_e], 1), ("seventeen", many, 1),
              ("second_fill", [s_a2, (576 + 3 * b + 2, 8, 9), (576 + 4 * b - 2, 34, 16), s_t], 2)]
    with_a = {1: {"A", "B"}, 2: {"A", "B", "C"}, 3: {"A", "B", "C", "D"}}
    joined = {c: {"one_in_A": with_a[c], "one_in_E": {"E", "F"}, "seventeen": with_a[c] | {"E", "F", "G", "G2", "T", "L"},
                  "second_fill": with_a[c] | {"H", "H2", "T"}} for c in (1, 2, 3)}
    # whole blocks for fill 1: every block of every body but E's short one and the one(s) its slab of 1s touches
    nblk = {k: -(-(v[2].stop - v[2].start) // b) for k, v in bodies.items()}
    nblk["E"] -= 1 + len({x // b for x in range(400, 410)})
    nblk["H2"] -= 1                                   # starts one voxel late
    nblk["T"] -= 1                                    # the tail
    for k in ("G", "H", "G2", "H2", "L"):             # both tile slices
        nblk[k] *= 2
    return Case(img, out0, floods, chained={"second_fill"}, bodies=bodies, joined=joined, block=b,
                whole_blocks=sum(nblk.values()), loose=loose,
                loose_share=float(loose.sum()) / float((~(ids > 0) & ~keep_out).sum()))


def body_counts(case, fill, before, after):
    """{body: (voxels the flood filled in it, its candidate voxels)}"""
    got = (after == fill) & (before != fill)
    c = (case.img >= T0) & (case.img <= T1) & (before != fill)
    return {k: (int(got[v].sum()), int(c[v].sum())) for k, v in case.bodies.items()}


# ---- (c) rows per lane and the LDS limit -----------------------------------------------------------------------------------
ROWS = {"rows65": (13, 5, 5), "rows1025": (41, 25, 5), "rows86x85": (86, 85, 3), "rows86x86": (86, 86, 3)}  # nty, ntz, dx


@functools.lru_cache(maxsize=None)
def rows_case(name):
    """dx of a few voxels, partial tiles on the high sides of y and z.  Tile row 0 (y < 16) is a second body, tile row 1 a
    non-candidate wall with loose voxels, tile rows 2.. one solid slab over every slice, so the slab owns the last row of
    tiles of every lane slot; the seed sits in the slab's first tile (slice 0), hops6 / hops26 tile hops from its far end
    by faces / with diagonal steps.  Two slabs of pre-filled voxels make two of the slab's tiles not whole."""
    nty, ntz, dx = ROWS[name]
    dy, dz = nty * TY - 7, ntz * TZ - 5
    img = np.zeros((dz, dy, dx), np.int16)
    bodies = {"slab": (slice(0, dz), slice(32, dy), slice(0, dx)), "behind": (slice(0, dz), slice(0, 16), slice(0, dx))}
    for v in bodies.values():
        img[v] = VAL
    wall = np.zeros(img.shape, bool)
    wall[:, 16:32, :] = True
    rng = np.random.default_rng(3000 + nty * ntz)
    loose = wall & (rng.random(img.shape) < 0.03)
    loose[:, 23:25, :] = False  # two empty planes in the middle: loose voxels touch either body, never both
    img[loose] = VAL
    out0 = np.zeros(img.shape, np.uint8)
    out0[dz // 2, 40:44, 1:2] = 1
    out0[dz - 2, dy - 3, :] = 1
    floods = [("slab", [(1, 36, 2)], 1), ("both", [(1, 36, 2), (0, 3, dz - 1)], 1)]
    joined = {c: {"slab": {"slab"}, "both": {"slab", "behind"}} for c in (1, 3)}
    return Case(img, out0, floods, bodies=bodies, joined=joined, rows=nty * ntz, hops6=(nty - 3) + (ntz - 1),
                hops26=max(nty - 3, ntz - 1))


# ---- (d) tile-level serpentine, all-candidate volumes ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tile_serpentine():
    """dz = 1, dx = 1100 (18 tiles per row, the last 12 voxels wide; block width 32): 30 corridors, each one row of whole
    tiles, between them 29 non-candidate tile rows with one whole tile at alternating ends.  The seed is at the low-x end
    of corridor 0; the far end is 30 * 17 + 29 * 2 tile hops away."""
    ncorr, dx = 30, 1100
    wx = -(-dx // TX)
    dy = (2 * ncorr - 1) * TY
    img = np.zeros((1, dy, dx), np.int16)
    for k in range(ncorr):
        img[0, 2 * k * TY:(2 * k + 1) * TY, :] = VAL
        if k + 1 < ncorr:
            x0 = (wx - 1) * TX if k % 2 == 0 else 0
            img[0, (2 * k + 1) * TY:(2 * k + 2) * TY, x0:x0 + TX] = VAL
    out0 = np.zeros(img.shape, np.uint8)
    return Case(img, out0, [("snake", [(3, 3, 0)], 1)], hops=ncorr * (wx - 1) + (ncorr - 1) * 2)


def tile_hops(case):
    """tile hops (face steps on the grid of all-candidate tiles) from the seed's tile to the farthest one, by dilation"""
    (_, seeds, _), = case.floods
    dz, dy, dx = case.shape
    assert dz == 1 and dy % TY == 0
    nx = -(-dx // TX)
    pad = np.ones((dy, nx * TX), bool)
    pad[:, :dx] = (case.img[0] >= T0) & (case.img[0] <= T1)
    whole = pad.reshape(dy // TY, TY, nx, TX).all(axis=(1, 3))
    x, y, _ = seeds[0]
    cur = np.zeros_like(whole)
    cur[y // TY, x // TX] = True
    assert whole[y // TY, x // TX]
    hops = 0
    while True:
        nxt = ndimage.binary_dilation(cur, structure=ndimage.generate_binary_structure(2, 1)) & whole
        if (nxt == cur).all():
            return hops, bool((cur == whole).all())
        cur, hops = nxt, hops + 1


ALL_CANDIDATE_WIDTHS = (1000, 2000, 4000)  # block widths 16, 32, 64


@functools.lru_cache(maxsize=None)
def all_candidate(dx):
    """(2, 40, dx): three tile rows, the last one partial; the seed in the middle"""
    img = np.full((2, 40, dx), VAL, np.int16)
    return Case(img, np.zeros(img.shape, np.uint8), [("all", [(dx // 2, 20, 1)], 1)], hops=dx // 2 // TX)


# ---- (e) lists longer than the grid, many seeds, ring wrap -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_list():
    """(2, 800, 3300): 52 x 50 x 1 = 2600 tiles, noise of density 0.62, 5000 seeds drawn from the in-range voxels"""
    shape = (2, 800, 3300)
    rng = np.random.default_rng(4000)
    img = np.where(rng.random(shape) < 0.62, VAL, 0).astype(np.int16)
    idx = np.argwhere(img == VAL)
    idx = idx[rng.choice(len(idx), 5000, replace=False)]
    seeds = [(int(x), int(y), int(z)) for z, y, x in idx]
    return Case(img, np.zeros(shape, np.uint8), [("many", seeds, 1)])


def woken_tiles(case):
    """tiles in the 3 x 3 x 3 tile neighbourhoods of the seeds: the first round's list when the start is not fused (no tile
    of this noise is all-candidate, so the coarse pass takes none of them away)"""
    (_, seeds, _), = case.floods
    dz, dy, dx = case.shape
    g = np.zeros((-(-dz // TZ), -(-dy // TY), -(-dx // TX)), bool)
    for x, y, z in seeds:
        g[z // TZ, y // TY, x // TX] = True
    return int(ndimage.binary_dilation(g, structure=np.ones((3, 3, 3), bool)).sum())


RING_TILES = 30


@functools.lru_cache(maxsize=None)
def ring_corridor():
    """(2, 3, 30 * 64 + 5): a voxel-wide line along x through 31 tiles, seeded at x = 0.  A visit closes a run inside its
    word at once and hands one bit to the next tile, which the next round visits: one round per tile."""
    shape = (2, 3, RING_TILES * TX + 5)
    img = np.zeros(shape, np.int16)
    img[1, 1, :] = VAL
    img[0, ::2, 7::9] = VAL  # specks that touch the line by an edge or a corner only
    return Case(img, np.zeros(shape, np.uint8), [("line", [(0, 1, 1)], 1)], tiles=RING_TILES + 1)
