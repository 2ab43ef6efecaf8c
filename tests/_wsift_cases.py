"""Case builders and a plain census for the level chain of the IFT watershed (csrc/k_wsift.hip, stages 3 to 5: entries by
level, keys / rank / claim per level, labels).  Nothing here imports the package under test: `census` restates in flat numpy
what the header of k_wsift.hip defines (parents, entries, zones, parent words) from the reference's cost map, so that every
case can say which branch of the chain it reaches (test_wsift_cases_host.py asserts it without a GPU) and so that the flood's
statistics have an independent expectation (test_gpu_wsift_chain.py).

The constants restated from the .hip files: USED_LDS_WORDS (the used-key bitmap lives in LDS while the stamps issued so far
fit 8192 words), the 1024 lanes of k_ws_rank, the 16384 voxels and the 4096 LDS counters of a bucket workgroup."""
import numpy as np
from scipy.ndimage import generate_binary_structure
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

USED_LDS_WORDS = 8192      # k_wsift.hip: ws_mark_used_block (LDS) while (base + 31) >> 5 <= this, ws_mark_used (per wave) above
USED_LDS_STAMPS = USED_LDS_WORDS * 32
RANK_LANES = 1024          # k_ws_rank: chunk = ceil(words / 1024) bitmap words per lane
BUCKET_VOXELS = 256 * 64   # ws_tiles.h: 256 lanes x BK_CH voxels per bucket workgroup
BUCKET_LDS_LEVELS = 4096   # ws_tiles.h: BK_LB, levels counted in LDS; higher ones go to the global cursor


def _offsets(structure, shape3):
    """linear offsets of the structuring element's set cells (centre excluded) in a (d, h, w) volume"""
    s = np.asarray(structure).astype(bool)
    s3 = np.zeros((3, 3, 3), bool)
    if s.ndim == 3:
        s3[:] = s
    else:
        s3[1] = s
    _, h, w = shape3
    return [(dz - 1) * h * w + (dy - 1) * w + (dx - 1)
            for dz in range(3) for dy in range(3) for dx in range(3) if s3[dz, dy, dx] and (dz, dy, dx) != (1, 1, 1)]


def _distinct_per_row(words):
    """number of distinct values >= 0 in every row of a 2-D int64 array (-1 = nothing there)"""
    if words.shape[0] == 0:
        return np.zeros(0, np.int64)
    s = np.sort(words, axis=1)
    first = np.concatenate([s[:, :1] >= 0, (s[:, 1:] != s[:, :-1]) & (s[:, 1:] >= 0)], axis=1)
    return first.sum(axis=1)


def census(img, markers, structure, cost):
    """What the reference's cost map `cost` (oracle.watershed_ift_clean(..., want_cost=True)) says about the flood of
    `img` from `markers`: a dict of
      markers       marker voxels
      entries       entries that are not markers
      levels        distinct cost values among them
      max_level     the largest of those (0 without any)
      level_counts  {cost: entries at that cost}
      parents_hist  [entries with 1, 2, more than 2 distinct parent words]
      zones_hist    [entries with 0, 1, 2, 3, more than 3 distinct zone roots among the non-entry voxels they touch]
      marker_classes  runs of equal label among the markers in raster order: the time stamps level 0 issues (k_ws_rank gives
                      one to each run, the FIRST run the highest), so that markers + marker_classes stamps exist when the first
                      level above 0 looks at the used-key bitmap
      top_stamp_is_key  an entry of the lowest level has all its parents among the markers of that first run: its key is the
                      highest stamp issued so far, the top bit of the bitmap that level sees
    Neighbours go by linear index (q = p + dz*hw + dy*w + dx, valid iff 0 <= q < n), as in scipy and in the kernel."""
    img = np.asarray(img)
    shape3 = img.shape if img.ndim == 3 else (1,) + img.shape
    I = img.reshape(-1).astype(np.int64)
    C = np.asarray(cost).reshape(-1).astype(np.int64)
    mk = np.asarray(markers).reshape(-1)
    n = I.size
    offs = _offsets(structure, shape3)
    p = np.arange(n, dtype=np.int64)
    is_marker = mk != 0

    par = np.zeros((len(offs), n), bool)    # neighbour k of p is a parent of p
    zon = np.zeros((len(offs), n), bool)    # neighbour k of p is zone-linked to p
    nbr = np.zeros((len(offs), n), np.int64)
    for k, o in enumerate(offs):
        q = p + o
        ok = (q >= 0) & (q < n)
        qc = np.where(ok, q, 0)
        w = np.abs(I[qc] - I)
        par[k] = ok & ~is_marker & (C[qc] < C) & (w == C)
        zon[k] = ok & (C[qc] == C) & (w <= C)
        nbr[k] = qc
    entry = is_marker | par.any(axis=0)

    # zones: components of non-entry voxels under zone links, root = smallest index
    rows, cols = [], []
    for k in range(len(offs)):
        sel = zon[k] & ~entry & ~entry[nbr[k]]
        rows.append(p[sel])
        cols.append(nbr[k][sel])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    _, comp = connected_components(coo_matrix((np.ones(rows.size, np.int8), (rows, cols)), shape=(n, n)), directed=False)
    root_of_comp = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(root_of_comp, comp, p)
    word = np.where(entry, p, root_of_comp[comp])  # the word of tau that holds a voxel's stamp

    ent = np.flatnonzero(entry & ~is_marker)
    pw = np.full((ent.size, len(offs)), -1, np.int64)
    zr = np.full((ent.size, len(offs)), -1, np.int64)
    for k in range(len(offs)):
        q = nbr[k][ent]
        pw[:, k] = np.where(par[k][ent], word[q], -1)
        zr[:, k] = np.where(zon[k][ent] & ~entry[q], word[q], -1)
    npar, nzon = _distinct_per_row(pw), _distinct_per_row(zr)
    assert ent.size == 0 or npar.min() >= 1
    lv, cnt = np.unique(C[ent], return_counts=True)
    mlab = mk[is_marker]
    top = False
    if ent.size and mlab.size:
        first_run = np.zeros(n, bool)  # the markers before the first change of label in raster order
        change = np.flatnonzero(mlab[1:] != mlab[:-1])
        first_run[np.flatnonzero(is_marker)[:(change[0] + 1) if change.size else mlab.size]] = True
        low = C[ent] == lv[0]
        inside = np.ones(ent.size, bool)
        for k in range(len(offs)):
            inside &= ~par[k][ent] | first_run[nbr[k][ent]]
        top = bool((low & inside).any())
    return dict(markers=int(is_marker.sum()), entries=int(ent.size), levels=int(lv.size), max_level=int(lv.max()) if lv.size else 0,
                level_counts={int(a): int(b) for a, b in zip(lv, cnt)},
                parents_hist=[int((npar == 1).sum()), int((npar == 2).sum()), int((npar > 2).sum())],
                zones_hist=[int((nzon == i).sum()) for i in range(4)] + [int((nzon > 3).sum())],
                marker_classes=int(1 + (mlab[1:] != mlab[:-1]).sum()) if mlab.size else 0, top_stamp_is_key=top)


# ---- builders: (uint16 image, int16 markers), both 3-D ------------------------------------------------------------------------
def star_lattice(shape, seed=0, walls=(1000, 9000)):
    """Made for the many-zones branch at 6-connectivity.  Lattice lines (at least two of z%3==0, y%3==0, x%4==0) have intensity
    10, everything else is wall (walls[0] + r left of w//2, walls[1] + r right of it, r random in {0, 1, 2}).  A centre has all
    three conditions true; the voxel at x%4==3 in front of a centre is a marker (intensity 0, random label 1..3).  The centre
    is then an entry of cost 10 whose other five neighbours are one- or two-voxel zones, each claimed by whichever of the two
    entries at its ends was popped first; the walls are large zones at two cost levels, one on either side of 4096."""
    rng = np.random.default_rng(seed)
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    on = (z % 3 == 0).astype(int) + (y % 3 == 0) + (x % 4 == 0)
    r = rng.integers(0, 3, shape)
    img = np.where(on >= 2, 10, np.where(x < w // 2, walls[0], walls[1]) + r).astype(np.uint16)
    centre = on == 3
    front = np.zeros(shape, bool)
    front[:, :, :-1] = centre[:, :, 1:]
    front &= x % 4 == 3
    mk = np.zeros(shape, np.int16)
    mk[front] = rng.integers(1, 4, int(front.sum()))
    img[front] = 0
    return img, mk


def checker_markers(shape, seed=0, levels=4):
    """markers of random label 1..3 on every voxel with (z+y+x)%2==0, intensities random in [0, levels): every other voxel
    has six marker neighbours, and so many tied parents"""
    rng = np.random.default_rng(seed)
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    img = rng.integers(0, levels, shape).astype(np.uint16)
    mk = np.where((z + y + x) % 2 == 0, rng.integers(1, 4, shape), 0).astype(np.int16)
    return img, mk


def dense_markers(shape, n_markers, seed=0, levels=40):
    """exactly n_markers marker voxels chosen without replacement, labels random in 1..3; the last voxel in raster order is one
    of them, so key n_markers - 1 -- the top of the last word of level 0's bitmap -- is in use.  Intensities random in
    [0, levels)."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    img = rng.integers(0, levels, shape).astype(np.uint16)
    mk = np.zeros(n, np.int16)
    if n_markers > 0:
        where = np.concatenate([rng.permutation(n - 1)[:n_markers - 1], [n - 1]])
        mk[where] = rng.integers(1, 4, n_markers)
    return img, mk.reshape(shape)


def dense_stamps(shape, stamps, seed=0, levels=40, share=0.6):
    """dense_markers with the number of time stamps that exist after level 0 fixed: m = int(stamps * share) marker voxels whose
    labels, read in raster order, form exactly stamps - m runs (a run of equal labels is one class of k_ws_rank, one stamp), so
    the first level above 0 sees a used-key bitmap of exactly `stamps` bits.  The corner is arranged so that the highest of them
    is a key of that level: voxel 0 is a marker (its run is the first, which gets the highest stamp), voxel 1 is not and differs
    from it by 1, and voxel 1's other neighbours are markers 9 away -- voxel 1 is an entry of cost 1 with voxel 0 its only parent."""
    rng = np.random.default_rng(seed)
    d, h, w = shape
    n = d * h * w
    m = int(stamps * share)
    runs = stamps - m
    assert 1 <= runs <= m <= n - 1 and d > 1 and h > 1 and w > 2
    img = rng.integers(0, levels, shape).astype(np.uint16).reshape(-1)
    forced = np.array([0, 2, 1 + w, 1 + h * w, n - 1])
    free = np.setdiff1d(np.arange(n), np.concatenate([forced, [1]]))
    where = np.sort(np.concatenate([forced, rng.permutation(free)[:m - forced.size]]))
    change = np.zeros(m, np.int64)  # 0: same label as the marker before; 1 or 2: one of the two others
    change[1 + rng.permutation(m - 1)[:runs - 1]] = rng.integers(1, 3, runs - 1)
    mk = np.zeros(n, np.int16)
    mk[where] = (np.cumsum(change) + int(rng.integers(0, 3))) % 3 + 1
    img[0], img[1], img[[2, 1 + w, 1 + h * w]] = 10, 11, 20
    return img.reshape(shape), mk.reshape(shape)


# One row per flood: id, builder, its arguments, the rank of the arrays handed over (2: the builder's single slice), the
# connectivity (scipy's generate_binary_structure rank), `need` = what the census must show for the case to reach the branch
# it is named for (minimum conditions, asserted by test_wsift_cases_host.py), `seen` = what the census gave for exactly this
# construction when the table was written (parents_hist = entries with 1 / 2 / >2 distinct parent words, zones_hist = entries
# touching 0 / 1 / 2 / 3 / >3 distinct zones; asserted too, so a retuned builder shows up there).
#
# Which rows close which gap (every row runs with and without the link records, so each also runs the unlinked chain):
#   star-*      LINK_MORE in k_ws_claim_links (more than 3 zones); star-3blocks-26 and checker*: LINK_MORE in k_ws_keys_links
#               (more than 2 parent words)
#   star-tiles, star-3blocks*   entries on both sides of the bucket's 4096 LDS counters; star-3blocks: three bucket workgroups,
#               the last one partial; in the star rows k_ws_bucket meets waves whose entries share one level (walls: its
#               one-atomic path) next to waves that mix a centre with walls, in the dense rows mostly mixed ones
#   rank-*      k_ws_rank at 1024 / 1025 bitmap words (level 0, the markers' own keys), two-word chunks afterwards
#   used-*      level 0 ranks 8192 / 8193 words.  Level 0 issues one stamp per run of equal marker labels -- about 2 m / 3 of
#               them for three random labels -- so every later level of these rows already sees more than 2^18 stamps: they
#               all run ws_mark_used, the per-wave loop, and none sits at the switch itself
#   stamps-*    markers + runs fixed instead: the first level above 0 sees exactly 2^18 - 4 / 2^18 / 2^18 + 1 stamps, with the
#               highest of them in use as a key: the LDS bitmap at its last word (8192), the per-wave loop at its first
#               (8193), and stamps-cross starts on the LDS bitmap and ends on the per-wave loop
def _row(id, build, args, ndim, conn, need, seen):
    return dict(id=id, build=build, args=args, ndim=ndim, conn=conn, need=need, seen=seen)


_BIG = (10, 168, 168)
WSIFT_CHAIN_CASES = [
    _row("star-1tile", star_lattice, ((7, 10, 13),), 3, 1, dict(zones_more=10, zones_1=3, zones_2=3, zones_3=3),
         dict(markers=36, entries=135, levels=3, parents_hist=[117, 18, 0], zones_hist=[0, 105, 4, 10, 16])),
    _row("star-tiles", star_lattice, ((13, 13, 21),), 3, 1, dict(zones_more=50, both_sides_of_lds_levels=True),
         dict(markers=125, entries=513, levels=3, parents_hist=[404, 102, 7], zones_hist=[0, 398, 6, 25, 84])),
    _row("star-3blocks", star_lattice, ((12, 40, 70),), 3, 1, dict(zones_more=500, bucket_blocks=3, both_sides_of_lds_levels=True),
         dict(markers=952, entries=4408, levels=3, parents_hist=[3371, 1019, 18], zones_hist=[0, 3454, 2, 34, 918])),
    _row("star-3blocks-26", star_lattice, ((12, 40, 70),), 3, 3, dict(parents_more=1000, bucket_blocks=3, both_sides_of_lds_levels=True),
         dict(markers=952, entries=9770, levels=3, parents_hist=[5165, 2000, 2605], zones_hist=[0, 9436, 334, 0, 0])),
    _row("checker", checker_markers, ((9, 17, 33),), 3, 1, dict(parents_more=200),
         dict(markers=2525, entries=489, levels=3, parents_hist=[76, 119, 294], zones_hist=[489, 0, 0, 0, 0])),
    _row("checker-2d", checker_markers, ((1, 40, 40),), 2, 1, dict(parents_more=50),
         dict(markers=800, entries=261, levels=3, parents_hist=[62, 102, 97], zones_hist=[261, 0, 0, 0, 0])),
    _row("rank-1024w", dense_markers, ((4, 96, 96), 32768), 3, 1, dict(markers=32768, levels=3, rank_words0=1024),
         dict(markers=32768, entries=3513, levels=25, parents_hist=[3109, 375, 29], zones_hist=[3395, 114, 4, 0, 0])),
    _row("rank-1025w", dense_markers, ((4, 96, 96), 32769), 3, 1, dict(markers=32769, levels=3, rank_words0=1025),
         dict(markers=32769, entries=3512, levels=25, parents_hist=[3108, 375, 29], zones_hist=[3394, 114, 4, 0, 0])),
    _row("used-cross", dense_markers, (_BIG, 2 ** 18 - 4), 3, 1, dict(levels=6),
         dict(markers=262140, entries=17250, levels=28, parents_hist=[15110, 1988, 152], zones_hist=[16853, 394, 3, 0, 0])),
    _row("used-8192w", dense_markers, (_BIG, 2 ** 18), 3, 1, dict(levels=3, parents_more=50, rank_words0=8192),
         dict(markers=262144, entries=17247, levels=28, parents_hist=[15109, 1986, 152], zones_hist=[16850, 394, 3, 0, 0])),
    _row("used-8193w", dense_markers, (_BIG, 2 ** 18 + 1), 3, 1, dict(levels=3, parents_more=50, rank_words0=8193),
         dict(markers=262145, entries=17246, levels=28, parents_hist=[15108, 1986, 152], zones_hist=[16849, 394, 3, 0, 0])),
    _row("stamps-cross", dense_stamps, (_BIG, 2 ** 18 - 4), 3, 1, dict(levels=6, stamps1=2 ** 18 - 4, top_stamp_is_key=True),
         dict(markers=157284, entries=94758, levels=32, parents_hist=[85386, 8794, 578], zones_hist=[79479, 14125, 1110, 43, 1])),
    _row("stamps-8192w", dense_stamps, (_BIG, 2 ** 18), 3, 1, dict(levels=3, stamps1=2 ** 18, top_stamp_is_key=True, parents_more=50),
         dict(markers=157286, entries=94757, levels=32, parents_hist=[85386, 8793, 578], zones_hist=[79479, 14124, 1110, 43, 1])),
    _row("stamps-8193w", dense_stamps, (_BIG, 2 ** 18 + 1), 3, 1, dict(levels=3, stamps1=2 ** 18 + 1, top_stamp_is_key=True, parents_more=50),
         dict(markers=157287, entries=94756, levels=32, parents_hist=[85385, 8793, 578], zones_hist=[79478, 14124, 1110, 43, 1])),
]
CASE_IDS = [c["id"] for c in WSIFT_CHAIN_CASES]


def build_case(case):
    """(image, markers, structure) as handed to the flood"""
    img, mk = case["build"](*case["args"])
    if case["ndim"] == 2:
        img, mk = img[0], mk[0]
    return img, mk, generate_binary_structure(case["ndim"], case["conn"])


def bitmap_words(stamps):
    return (stamps + 31) >> 5


def check_need(case, cen, shape):
    """assert the row's minimum conditions on a census"""
    need = case["need"]
    ph, zh = cen["parents_hist"], cen["zones_hist"]
    got = dict(markers=cen["markers"], stamps1=cen["markers"] + cen["marker_classes"], top_stamp_is_key=cen["top_stamp_is_key"],
               rank_words0=bitmap_words(cen["markers"]), bucket_blocks=-(-int(np.prod(shape)) // BUCKET_VOXELS),
               both_sides_of_lds_levels=min(cen["level_counts"]) < BUCKET_LDS_LEVELS <= max(cen["level_counts"]))
    atleast = dict(levels=cen["levels"], parents_more=ph[2], zones_more=zh[4], zones_1=zh[1], zones_2=zh[2], zones_3=zh[3])
    for k, v in need.items():
        if k in got:
            assert got[k] == v, (case["id"], k, got[k], v)
        else:
            assert atleast[k] >= v, (case["id"], k, atleast[k], v)
