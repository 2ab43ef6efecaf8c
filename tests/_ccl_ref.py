"""Inputs and plain numpy / scipy references for the run-based union-find of csrc/k_ccl.hip (tests/test_gpu_ccl.py on
the GPU, tests/test_ccl_cases_host.py anywhere).  Test infrastructure only: the product never imports it.

The engine works on tiles of 8 words (512 voxels) x 8 rows x 4 slices and scans 4096 words per workgroup, so every case
here is 1030 voxels wide: 17 words per row, the last with 6 valid bits, three tiles along x.

    noise(conn) / checker() / solid() / stairs() / edges()    the imask patterns P (bool, z y x) of cases A..E
    pattern(case, conn)                                       the same by name
    mask_of(P)                                                the padded uint8 mask matrix whose imask is P
    fill_holes(matrix, target, conn, orientation, index, size)  Mask.fill_holes_auto restated -> (matrix, changed)
    known_groups(case, conn)                                  B..E: the components as they were BUILT, no labelling
    fill_holes_known(P, groups, size)                         the same rule applied to those -> (inner, changed)
    fill_sizes(case, conn)                                    the sizes the tests run per case
    indices_2d(case, orientation) / sizes_2d(case)            the slices and sizes of the 2-D paths
    straddling(labels, axis, lo)                              labels with voxels at index <= lo and > lo of an axis
    flood_seeds(P, conn) / flood_barriers(shape, seed)        seeds (x, y, z) and a pre-filled out array for the floods
    flood_by_label(P, seeds, fill, strct, out0)               "the labelled components that hold an in-range seed"
    serpentine()                                              the (3, 60, 1100) corridor that needs hundreds of tile hops
"""
import functools

import numpy as np
from scipy import ndimage

WIDE = 1030  # 16 whole words + 6 bits; x tile boundaries at 511|512 and 1023|1024
SHAPES = {"noise": (10, 25, WIDE), "checker": (5, 9, WIDE), "solid": (5, 9, WIDE), "stairs": (8, 16, WIDE),
          "edges": (5, 9, WIDE)}
CASES = tuple(SHAPES)
RANK = {4: 1, 8: 2, 6: 1, 18: 2, 26: 3}
DENSITY = {6: 0.30, 18: 0.15, 26: 0.10}  # below the site-percolation threshold of each neighbourhood: many components
SIZE_A = 5
CHAIN = 4  # voxels per chain of case D


def structure(conn):
    return ndimage.generate_binary_structure(3, RANK[conn])


# ---- the cases --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise(conn):
    """A: 17 words per row, 3 x 4 x 3 tiles with a partial one on every high side, 4250 words = two scan blocks"""
    p = np.random.default_rng(7100 + conn).random(SHAPES["noise"]) < DENSITY[conn]
    p.setflags(write=False)
    return p


def checker():
    """B: 32 runs in every whole word, 8192 local nodes in a whole tile; 23175 voxels"""
    z, y, x = np.indices(SHAPES["checker"])
    return (x + y + z) % 2 == 0


def solid():
    """C: every word one 64-bit run that continues into the next word; two slabs of 2 * 9 * 1030 voxels"""
    p = np.ones(SHAPES["solid"], bool)
    p[2] = False
    return p


def stairs_chains():
    """D: one-voxel chains of CHAIN voxels, [(kind, (CHAIN, 3) int array of z, y, x)].  kind "zyx" steps in all three
    axes at once (one component under 26 only), "yx" and "zx" in two (one component under 18 and 26).  Around each of
    the x boundaries 191|192 (words inside a tile), 511|512 and 1023|1024 (words of two tiles):
      * one "zyx" chain whose middle step crosses x, y = 7 -> 8 and z = 3 -> 4 together: x increasing at 512, x
        decreasing at 192 and 1024 (the two directions cannot both be had at one boundary: their crossing steps lie in
        the same 2 x 2 x 2 cube and would touch);
      * a pair of "zyx" chains, x increasing and decreasing, with y and z inside one tile;
      * pairs of "yx" chains crossing y = 7 -> 8 and of "zx" chains crossing z = 3 -> 4 at the same x step."""
    k = np.arange(CHAIN)
    chains = []

    def add(kind, z, y, x):
        chains.append((kind, np.stack([z + 0 * k, y + 0 * k, x + 0 * k], 1)))

    for b, triple_up in ((192, False), (512, True), (1024, False)):
        up, down = b - 2 + k, b + 1 - k  # x = b-1 -> b at the middle step, and b -> b-1
        add("zyx", 2 + k, 6 + k, up if triple_up else down)
        add("zyx", k, 1 + k, up)          # z 0..3, y 1..4: one tile
        add("zyx", 4 + k, 11 + k, down)   # z 4..7, y 11..14: one tile
        add("yx", 0, 6 + k, up)
        add("yx", 7, 6 + k, down)
        add("zx", 2 + k, 0, up)
        add("zx", 2 + k, 15, down)
    return chains


def _paint(shape, voxels):
    p = np.zeros(shape, bool)
    p[tuple(np.asarray(voxels).T)] = True
    return p


def stairs():
    return _paint(SHAPES["stairs"], np.concatenate([v for _, v in stairs_chains()]))


def edge_bars():
    """E: isolated bars on an empty background, [(name, (n, 3) int array of z, y, x)]"""
    def row(z, y, x0, x1):
        x = np.arange(x0, x1 + 1)
        return np.stack([0 * x + z, 0 * x + y, x], 1)

    ell = np.array([(3, 4, 100), (3, 5, 100), (3, 6, 100), (3, 7, 100), (3, 8, 100), (4, 8, 100), (4, 8, 101)])
    return [("last_word", row(1, 2, 1024, 1029)),   # 6: the whole valid part of the last word
            ("bar600", row(1, 4, 200, 799)),        # 600: 11 words, across the tile boundary at 512
            ("bar599", row(3, 1, 431, 1029)),       # 599: across both tile boundaries, up to the last valid bit
            ("ell7", ell),                          # 7: wraps the corner y 7 -> 8, z 3 -> 4
            ("origin5", row(0, 0, 0, 4)),
            ("word6", row(0, 3, 61, 66)),           # 6: across a word boundary inside a tile
            ("tile5", row(0, 7, 510, 514)),         # 5: across the tile boundary
            ("tail5", row(4, 4, 1022, 1026)),       # 5: across the last tile boundary into the partial word
            ("corner1", row(4, 8, 1029, 1029))]     # 1: the far corner


def edges():
    return _paint(SHAPES["edges"], np.concatenate([v for _, v in edge_bars()]))


def pattern(case, conn):
    return noise(conn) if case == "noise" else {"checker": checker, "solid": solid, "stairs": stairs, "edges": edges}[case]()


def pattern_2d(case, conn):
    """the 3-D pattern the 2-D paths (4 / 8) slice: A at the density of 6 / 18"""
    return pattern(case, {4: 6, 8: 18}[conn])


def mask_of(p):
    m = np.zeros(tuple(s + 1 for s in p.shape), np.uint8)
    m[1:, 1:, 1:] = np.where(p, 0, 255)
    return m


# ---- Mask.fill_holes_auto ---------------------------------------------------------------------------------------------
def view_of(matrix, target, orientation, index):
    if target == "3D":
        return matrix[1:, 1:, 1:]
    return {"AXIAL": lambda: matrix[index + 1, 1:, 1:], "CORONAL": lambda: matrix[1:, index + 1, 1:],
            "SAGITAL": lambda: matrix[1:, 1:, index + 1]}[orientation]()


def fill_holes(matrix, target, conn, orientation, index, size):
    """invesalius/data/mask.py:519-562 with fill_holes_automatically (invesalius_rs/src/floodfill.rs:51-94) in numpy.
    Returns (a new matrix, whether anything was to be changed)."""
    out = matrix.copy()
    view = view_of(out, target, orientation, index)
    imask = ~(view > 127)
    labels, nlabels = ndimage.label(imask, ndimage.generate_binary_structure(view.ndim, RANK[conn]))
    if nlabels == 0:
        return out, False
    counts = np.bincount(labels.ravel(), minlength=nlabels + 1)
    if not ((counts > 0) & (counts <= size)).any():
        return out, False
    view[counts[labels] <= size] = 254
    return out, True


def known_groups(case, conn):
    """B..E: [(voxels per component, bool array of all the components of that size)] from how the case was built"""
    if case == "checker":
        p = checker()
        return [(1 if conn == 6 else int(p.sum()), p)]
    if case == "solid":
        p = solid()
        lo, hi = p.copy(), p.copy()
        lo[2:], hi[:3] = False, False
        return [(int(lo.sum()), lo), (int(hi.sum()), hi)]
    if case == "stairs":
        joined = {6: (), 18: ("yx", "zx"), 26: ("yx", "zx", "zyx")}[conn]
        groups = {1: [], CHAIN: []}
        for kind, v in stairs_chains():
            groups[CHAIN if kind in joined else 1].append(v)
        return [(n, _paint(SHAPES["stairs"], np.concatenate(v))) for n, v in groups.items() if v]
    if case == "edges":
        return [(len(v), _paint(SHAPES["edges"], v)) for _, v in edge_bars()]
    return None


def fill_holes_known(p, groups, size):
    """the rule of floodfill.rs:51-94 on components known by construction -> (the mask without its padding, changed)"""
    inner = np.where(p, 0, 255).astype(np.uint8)
    n0 = int((~p).sum())  # label 0: the voxels > 127
    if not (any(0 < n <= size for n, _ in groups) or 0 < n0 <= size):
        return inner, False
    for n, where in groups:
        if n <= size:
            inner[where] = 254
    if n0 <= size:
        inner[~p] = 254
    return inner, True


@functools.lru_cache(maxsize=None)
def labelled(case, conn):
    """(labels, counts) of a case under a 3-D connectivity"""
    labels, n = ndimage.label(pattern(case, conn), structure(conn))
    return labels, np.bincount(labels.ravel(), minlength=n + 1)


def fill_sizes(case, conn):
    if case == "noise":
        return [1, SIZE_A, SIZE_A + 1, int(labelled(case, conn)[1][1:].max()) + 1]
    if case == "checker":
        return [1, 23174, 23175]
    if case == "solid":
        return [9269, 9270, 18539, 18540]  # label 0 is the plane of 9270 voxels, each slab has 18540
    if case == "stairs":
        return [1, CHAIN - 1, CHAIN]
    return [5, 6, 7, 599, 600]


def indices_2d(case, orientation):
    """first, a middle and the last slice; the middle sagittal one is x = 512, which the chains of D cross"""
    dz, dy, dx = SHAPES[case]
    n = {"AXIAL": dz, "CORONAL": dy, "SAGITAL": dx}[orientation]
    return [0, 512 if orientation == "SAGITAL" else n // 2, n - 1]


def sizes_2d(case):
    return [SIZE_A] if case == "noise" else [1, CHAIN - 1, CHAIN]


def straddling(labels, axis, lo):
    """the labels (> 0) that have voxels at index <= lo and at index > lo of `axis`"""
    a = np.moveaxis(labels, axis, 0)
    both = np.intersect1d(np.unique(a[:lo + 1]), np.unique(a[lo + 1:]))
    return both[both > 0]


# ---- floods -----------------------------------------------------------------------------------------------------------
def flood_seeds(p, conn):
    """(x, y, z) seeds: the largest component, up to two components on both sides of each x tile boundary, a voxel
    outside the range and the two far corners"""
    labels, n = ndimage.label(p, structure(conn))
    counts = np.bincount(labels.ravel(), minlength=n + 1)
    want = [int(np.argmax(counts[1:])) + 1] if n else []
    for lo in (511, 1023):
        want += [int(v) for v in straddling(labels, 2, lo)[:2]]
    seeds = []
    for lab in dict.fromkeys(want):
        z, y, x = np.argwhere(labels == lab)[-1]
        seeds.append((int(x), int(y), int(z)))
    z, y, x = np.argwhere(~p)[len(p) // 2] if not p.all() else (0, 0, 0)
    dz, dy, dx = p.shape
    return seeds + [(int(x), int(y), int(z)), (0, 0, 0), (dx - 1, dy - 1, dz - 1)]


def flood_barriers(shape, seed):
    """a pre-filled out array: the voxels that already hold the fill value 1 are barriers, other values are not"""
    rng = np.random.default_rng(seed)
    out = np.where(rng.random(shape) < 0.02, 1, 0).astype(np.uint8)
    out[rng.random(shape) < 0.02] = 7
    return out


def flood_by_label(inrange, seeds, fill, strct, out0):
    """generic_floodfill_threshold (floodfill.rs:96-166) for a symmetric element, stated with scipy.ndimage.label: the
    candidates are the in-range voxels that do not hold `fill` yet, plus the in-range seeds (a seed is expanded
    whatever `out` holds there); `fill` goes to every candidate component that holds an in-range seed."""
    seeded = np.zeros(inrange.shape, bool)
    for x, y, z in seeds:
        seeded[z, y, x] = inrange[z, y, x]
    labels, _ = ndimage.label(inrange & ((out0 != fill) | seeded), strct)
    hit = np.unique(labels[seeded])
    out = out0.copy()
    out[np.isin(labels, hit[hit > 0])] = fill
    return out


def serpentine():
    """int16 image (3, 60, 1100): a one-voxel corridor of value 1 snaking through the z = 1 plane, 18 flood tiles per
    row and 30 rows (hundreds of tile hops, far past the 48 rounds after which the frontier hands over to the
    union-find), across both 512-voxel boundaries; specks in z = 2, some over a corridor row (joined under every element),
    some over the rows between (joined by a diagonal only)"""
    dz, dy, dx = 3, 60, 1100
    img = np.zeros((dz, dy, dx), np.int16)
    for y in range(0, dy, 2):
        img[1, y, :] = 1
        if y + 1 < dy:
            img[1, y + 1, dx - 1 if (y // 2) % 2 == 0 else 0] = 1
    img[2, ::7, ::5] = 1
    return img
