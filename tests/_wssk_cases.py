"""A plain reference, a census and case builders for the level chain of the GUI-default watershed (csrc/k_wssk.hip, stage 3:
per non-empty level, ascending -- a run of small levels in one workgroup, a basin-free level relaxed tile-wise, or the level's
rounds in one resident launch).  Nothing here imports the package under test.

`flood` is the flood as the header of k_wssk.hip states it, in Python with heapq: cost C = minimax of the image values on a
path from a marker (markers: C = I); level c = {C == c}; GEN 0 = the level's markers in raster order, then the voxels of value
c with a neighbour of lower C, ordered by the smallest time among those neighbours; STEPS: one generation INTO a voxel of
value c, none INTO a lower one; TIME T = (G, R); label = label of the generation-0 ancestor R.  `census` counts from its
result what the chain's host code counts (lhist, hist, dhist of SkCtx), which kind of level the chain picks under given knobs,
and what the statistics of a call must then be.

Restated from k_wssk.hip -- test_wssk_cases_host.py looks every one of them up in the file's text, so a retune fails there
instead of silently moving a case off its path:
  SMALL_GEN0 = 4096, SMALL_TOTAL = 32768 and SkCtx::is_small (hist <= SMALL_GEN0 and lhist <= SMALL_TOTAL, unless IVX_SK_SMALL=0)
  SkCtx::is_tile_level (no drained voxel, lhist >= IVX_SK_TILE_LEVEL, default 1 << 16, 0 = never); is_small is asked first
  WB_CAP = 1024 (a wave's staged appends per pass), SK_SOLO_MAX = 256 (IVX_SK_SOLO's default), the default 256 of IVX_SK_PER_WG
  PSEQ_MOD = 0x3FF (sequence numbers of the resident launch's control word), LATE_MAX = 12000
  sk_carve_kind's grant of late-part key records: 6 neighbours, n >= n / 8 + 1024 + 2 * late_bytes + (1 << 22) with late_bytes =
  32 * late_max rounded up to 256; SkCarve::small_recs: 6 neighbours, rec_off + 32 * entries + 2 * late_bytes + 512 <= n with
  rec_off = (n / 8 + 511) & ~255
  the tied-marker count (k_sk_mixed, k_sk_levels_small): changes of label along a level's markers taken in raster order
  the tile 16 x 16 x 8 of ws_tiles.h (the builders put markers on its faces)"""
import heapq

import numpy as np
from scipy.ndimage import generate_binary_structure, morphological_gradient

SMALL_GEN0 = 4096
SMALL_TOTAL = 32768
WB_CAP = 1024
SK_SOLO_MAX = 256
PER_WG = 256
PSEQ_MOD = 0x3FF
LATE_MAX = 12000
TILE_LEVEL = 1 << 16
LATE_SLACK = 1 << 22
TX, TY, TZ = 16, 16, 8
WAVE = 64
_INF = 1 << 62


def _offsets3(structure):
    s = np.asarray(structure).astype(bool)
    s3 = np.zeros((3, 3, 3), bool)
    if s.ndim == 3:
        s3[:] = s
    else:
        s3[1] = s
    return [(k // 9 - 1, (k // 3) % 3 - 1, k % 3 - 1) for k in range(27) if s3.ravel()[k] and k != 13]


def flood(img, markers, structure):
    """The flood of the header of k_wssk.hip.  Returns a dict: labels (int32, the image's shape), cost (int64, 65535 where no
    marker reaches), G and R (the two halves of T, -1 where unreached; flat, raster order) and generations (the first
    generation a further level would get: what the library reports as stats["generations"])."""
    img = np.asarray(img)
    shape3 = img.shape if img.ndim == 3 else (1,) + img.shape
    d, h, w = shape3
    P = (d + 2, h + 2, w + 2)  # one cell of padding (value -1: nobody steps there) instead of bounds checks
    Ip = np.full(P, -1, np.int64)
    Ip[1:-1, 1:-1, 1:-1] = img.reshape(shape3)
    Mp = np.zeros(P, np.int64)
    Mp[1:-1, 1:-1, 1:-1] = np.asarray(markers).reshape(shape3)
    I, M = Ip.ravel().tolist(), Mp.ravel().tolist()
    offs = [(dz * P[1] + dy) * P[2] + dx for dz, dy, dx in _offsets3(structure)]
    N = len(I)
    # cost: Dijkstra with max as the path cost
    C = [_INF] * N
    heap = []
    for p in range(N):
        if M[p]:
            C[p] = I[p]
            heap.append((I[p], p))
    heapq.heapify(heap)
    while heap:
        c, p = heapq.heappop(heap)
        if c != C[p]:
            continue
        for o in offs:
            q = p + o
            v = I[q]
            if v < 0 or M[q]:
                continue
            nc = c if c > v else v
            if nc < C[q]:
                C[q] = nc
                heapq.heappush(heap, (nc, q))
    by_level = {}
    for p in range(N):
        if C[p] < _INF:
            by_level.setdefault(C[p], []).append(p)  # (raster order)
    tau = [_INF] * N  # (G << 32) | R
    lab = [0] * N
    runlabel = []
    gbase = 1
    for c in sorted(by_level):
        gen0 = []
        for p in by_level[c]:
            if I[p] != c:
                continue
            if M[p]:
                gen0.append((0, p, p, M[p]))  # markers first, in raster order
                continue
            best = _INF
            for o in offs:
                q = p + o
                if C[q] < c and tau[q] < best:  # (padding: C = _INF)
                    best = tau[q]
            if best < _INF:
                gen0.append((1, best, p, runlabel[best & 0xFFFFFFFF]))
        gen0.sort()
        front = []
        for _, _, p, l in gen0:
            tau[p] = (gbase << 32) | len(runlabel)
            runlabel.append(l)
            lab[p] = l
            front.append((tau[p], p))
        heapq.heapify(front)
        gmax = gbase
        while front:
            t, p = heapq.heappop(front)
            if t != tau[p]:
                continue
            gmax = max(gmax, t >> 32)
            for o in offs:
                q = p + o
                if C[q] != c or tau[q] <= t:
                    continue
                nt = t + ((1 << 32) if I[q] == c else 0)
                if nt < tau[q]:
                    tau[q] = nt
                    lab[q] = runlabel[nt & 0xFFFFFFFF]
                    heapq.heappush(front, (nt, q))
        gbase = gmax + 1
    inner = (slice(1, -1),) * 3
    tau = np.array([t if t < _INF else -1 for t in tau], np.int64).reshape(P)[inner].ravel()
    cost = np.minimum(np.array(C, np.int64), 65535).reshape(P)[inner].reshape(img.shape)
    return dict(labels=np.array(lab, np.int32).reshape(P)[inner].reshape(img.shape), cost=cost,
                G=np.where(tau < 0, -1, tau >> 32), R=np.where(tau < 0, -1, tau & 0xFFFFFFFF), generations=gbase)


def _has_lower_neighbour(C3, structure):
    d, h, w = C3.shape
    Cp = np.full((d + 2, h + 2, w + 2), _INF, np.int64)
    Cp[1:-1, 1:-1, 1:-1] = C3
    low = np.zeros(C3.shape, bool)
    for dz, dy, dx in _offsets3(structure):
        low |= Cp[1 + dz:1 + dz + d, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w] < C3
    return low


def tied_markers(img, markers):
    """what stats["tied_markers_of_different_labels"] counts: per image value, the changes of label along the markers of that
    value in raster order (0: the flood is scikit-image's own by construction)"""
    I, M = np.asarray(img).ravel().astype(np.int64), np.asarray(markers).ravel().astype(np.int64)
    at = np.flatnonzero(M)
    at = at[np.argsort(I[at], kind="stable")]
    return int(((I[at][1:] == I[at][:-1]) & (M[at][1:] != M[at][:-1])).sum())


def census(img, markers, structure, ref=None):
    """What the chain's host code counts, from the plain reference (`ref` = flood(...) if it is at hand): a dict of
      levels       one dict per non-empty level, ascending: c, voxels (lhist), gen0 (hist), drained (dhist), depth (generation
                   steps of the level: it uses depth + 1 generations), fronts (voxels of value c stamped per generation),
                   basin_gens (the generations, counted from the level's first, in which a basin is first stamped)
      generations  as flood()'s;  generation0  the sum of gen0;  tied  tied_markers()
      ref          the reference's result"""
    img = np.asarray(img)
    ref = ref or flood(img, markers, structure)
    shape3 = img.shape if img.ndim == 3 else (1,) + img.shape
    I = img.reshape(-1).astype(np.int64)
    C = ref["cost"].reshape(-1)
    G = ref["G"]
    M = np.asarray(markers).reshape(-1) != 0
    low = _has_lower_neighbour(C.reshape(shape3), structure).ravel()
    reached = G >= 0
    gen0 = reached & (M | ((I == C) & low))
    levels = []
    for c in np.unique(C[reached]).tolist():
        at = reached & (C == c)
        plateau, drained = at & (I == c), at & (I < c)
        g = G[plateau]
        g0 = int(g.min())
        assert (G[at & gen0] == g0).all() and (at & gen0).any()
        levels.append(dict(c=c, voxels=int(at.sum()), gen0=int((at & gen0).sum()), drained=int(drained.sum()),
                           depth=int(g.max()) - g0, fronts=np.bincount(g - g0).tolist(),
                           basin_gens=sorted(set((G[drained] - g0).tolist()))))
    assert ref["generations"] == 1 + sum(l["depth"] + 1 for l in levels)
    return dict(levels=levels, generations=ref["generations"], generation0=int(gen0.sum()), tied=tied_markers(img, markers), ref=ref)


def knobs_of(env):
    """the switches of sk_read_knobs that pick a level's path, from a dict of environment variables"""
    per_wg = int(env.get("IVX_SK_PER_WG", PER_WG))
    return dict(small_on=env.get("IVX_SK_SMALL", "1")[0] != "0", tile_min=int(env.get("IVX_SK_TILE_LEVEL", TILE_LEVEL)),
                solo_max=int(env.get("IVX_SK_SOLO", SK_SOLO_MAX)), per_wg=per_wg if per_wg >= 32 else PER_WG,
                late_max=min(int(env.get("IVX_SK_LATE_MAX", LATE_MAX)), LATE_MAX), late_recs=env.get("IVX_SK_LATE_RECS", "1")[0] != "0",
                small_recs=env.get("IVX_SK_SMALL_RECS", "1")[0] != "0", split=env.get("IVX_SK_SPLIT", "1")[0] != "0")


def level_kind(level, k):
    """'small', 'tile' or 'resident': SkCtx::is_small is asked first, then is_tile_level"""
    if k["small_on"] and level["gen0"] <= SMALL_GEN0 and level["voxels"] <= SMALL_TOTAL:
        return "small"
    if level["drained"] == 0 and k["tile_min"] and level["voxels"] >= k["tile_min"]:
        return "tile"
    return "resident"


def handover(level, solo_max):
    """The resident launch of one level: (words, longest): the control words published after the level's first (one per round
    that is handed over; the word that ends the level is the last) and the most generations begun between two of them (a
    solo stretch).  A round: A with the generation's frontier, then B with the level's drained voxels if a basin was stamped."""
    rounds = []  # (entries of the round, it begins a generation)
    for g, n in enumerate(level["fronts"]):
        rounds.append((n, g > 0))
        if g in level["basin_gens"]:
            rounds.append((level["drained"], False))
    words, longest, run = 0, 0, 0
    for n, begins in rounds[1:]:
        run += begins
        if n > solo_max:  # handed over: a word
            words += 1
            longest, run = max(longest, run), 0
    return words + 1, max(longest, run)


def chain(cen, env):
    """what a call under `env` must report: kinds (per level), small_level_runs, tile (any tile-wise level), and the resident
    levels' frontier_launches (rounds that did work), generation_steps and basin_rounds -- a resident level of depth D with B
    basin generations runs D + 1 A rounds and B relays, and begins D generations after its first"""
    k = knobs_of(env)
    kinds = [level_kind(l, k) for l in cen["levels"]]
    res = [l for l, kd in zip(cen["levels"], kinds) if kd == "resident"]
    runs = sum(1 for i, kd in enumerate(kinds) if kd == "small" and (i == 0 or kinds[i - 1] != "small"))
    return dict(kinds=kinds, small_level_runs=runs, tile="tile" in kinds, resident_levels=len(res),
                generation_steps=sum(l["depth"] for l in res), basin_rounds=sum(len(l["basin_gens"]) for l in res),
                frontier_launches=sum(l["depth"] + 1 + len(l["basin_gens"]) for l in res),
                handover=[handover(l, k["solo_max"]) for l in res])


def first_round_wave_appends(img, markers, structure, cen, c):
    """Per wave (64 consecutive entries of level c's sorted generation 0), the voxels it is CERTAIN to append in the level's
    first round: the unstamped voxels of value c that touch generation-0 voxels of this wave and of no other (a voxel touched
    by two waves is appended by whichever offer lands first)."""
    img = np.asarray(img)
    shape3 = img.shape if img.ndim == 3 else (1,) + img.shape
    d, h, w = shape3
    I = img.reshape(-1).astype(np.int64)
    C, G, R = cen["ref"]["cost"].reshape(-1), cen["ref"]["G"], cen["ref"]["R"]
    lv = (C == c) & (G >= 0)
    g0 = int(G[lv & (I == c)].min())
    gen0 = np.flatnonzero(lv & (I == c) & (G == g0))
    gen0 = gen0[np.argsort(R[gen0])]
    owner = {}
    for i, p in enumerate(gen0.tolist()):
        z, r = divmod(p, h * w)
        y, x = divmod(r, w)
        for dz, dy, dx in _offsets3(structure):
            a, b, e = z + dz, y + dy, x + dx
            if 0 <= a < d and 0 <= b < h and 0 <= e < w:
                q = (a * h + b) * w + e
                if C[q] == c and I[q] == c and G[q] == g0 + 1:
                    owner.setdefault(q, set()).add(i // WAVE)
    waves = [0] * (-(-gen0.size // WAVE))
    for q, s in owner.items():
        if len(s) == 1:
            waves[next(iter(s))] += 1
    return waves


def late_records_granted(n, conn, env=None):
    """sk_carve_kind: the late parts' key records fit into the n bytes of kind[]"""
    k = knobs_of(env or {})
    late_bytes = (k["late_max"] * 32 + 255) & ~255
    return k["late_recs"] and k["split"] and conn == 6 and n >= n // 8 + 1024 + 2 * late_bytes + LATE_SLACK


def small_records_granted(n, conn, entries, env=None):
    """SkCarve::small_recs: a run of `entries` generation-0 voxels gets its key records"""
    k = knobs_of(env or {})
    late_bytes = (k["late_max"] * 32 + 255) & ~255
    rec_off = (n // 8 + 511) & ~255
    return k["small_recs"] and conn == 6 and entries > 0 and rec_off + entries * 32 + 2 * late_bytes + 512 <= n


def level_table(img, cost, markers, structure):
    """The chain's histograms from a cost map alone, vectorised (the large case has no plain reference): per non-empty level, ascending,
    a dict of c, voxels, gen0, drained as in census(), and late: the generation-0 voxels that are no markers and whose neighbours of
    lower cost all lie in the next lower level that has voxels (k_sk_classify with k_sk_prevlevel's table)."""
    img = np.asarray(img)
    shape3 = img.shape if img.ndim == 3 else (1,) + img.shape
    d, h, w = shape3
    I3, C3 = img.reshape(shape3).astype(np.int32), np.asarray(cost).reshape(shape3).astype(np.int32)
    M3 = np.asarray(markers).reshape(shape3) != 0
    Cp = np.full((d + 2, h + 2, w + 2), 1 << 30, np.int32)
    Cp[1:-1, 1:-1, 1:-1] = C3
    minlow = np.full(shape3, 1 << 30, np.int32)  # the smallest cost among the neighbours of lower cost
    for dz, dy, dx in _offsets3(structure):
        q = Cp[1 + dz:1 + dz + d, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        minlow = np.where(q < C3, np.minimum(minlow, q), minlow)
    reached = C3 < 65535
    lhist = np.bincount(C3[reached], minlength=65536)
    prevl = np.full(65536, -1, np.int64)
    last = -1
    for c in np.flatnonzero(lhist).tolist():
        prevl[c] = last
        last = c
    gen0 = reached & (M3 | ((I3 == C3) & (minlow < (1 << 30))))
    late = gen0 & ~M3 & (minlow == prevl[C3])
    hist, hist_l = np.bincount(C3[gen0], minlength=65536), np.bincount(C3[late], minlength=65536)
    dhist = np.bincount(C3[reached & (I3 < C3)], minlength=65536)
    return [dict(c=c, voxels=int(lhist[c]), gen0=int(hist[c]), drained=int(dhist[c]), late=int(hist_l[c])) for c in np.flatnonzero(hist).tolist()]


def late_record_levels(table, n, conn, env=None):
    """The levels of a level_table whose late part is keyed from records: level cn is queued beside the level c below it when c
    took the stamping path (not a small run) and cn is neither small nor tile-wise, has an early part, and its late part is at
    most half of its generation 0 (sk_queue_early_after); the records are made when they are granted (n voxels, conn
    neighbours) and the late part has 1 .. late_max entries."""
    k = knobs_of(env or {})
    if not late_records_granted(n, conn, env):
        return []
    out, below_stamped = [], False
    for lv in table:
        kind = level_kind(lv, k)
        if below_stamped and kind == "resident" and lv["gen0"] - lv["late"] > 0 and lv["late"] <= lv["gen0"] // 2 and 0 < lv["late"] <= k["late_max"]:
            out.append(lv["c"])
        below_stamped = kind != "small"
    return out


def chain_of_table(table, env):
    """kinds, small_level_runs, tile and resident_levels as chain() gives them, from a level_table"""
    k = knobs_of(env)
    kinds = [level_kind(l, k) for l in table]
    runs = sum(1 for i, kd in enumerate(kinds) if kd == "small" and (i == 0 or kinds[i - 1] != "small"))
    return dict(kinds=kinds, small_level_runs=runs, tile="tile" in kinds, resident_levels=kinds.count("resident"))


# ---- builders: (image, markers), both 3-D unless stated ----------------------------------------------------------------------------
# No two labels ever share an image value among the markers: the tied-marker count counts the changes of label along a level's
# markers in raster order, whether the markers touch or not (the exception, lattice-overflow, is discussed at its row).
CORRIDOR, PIT, WALL = 10, 5, 20


def serpentine(h, w):
    """(y, x) of a one-voxel-wide corridor from (0, 0): the even rows 0 .. h - 2 in alternating direction, joined at their ends"""
    path = []
    rows = list(range(0, h - 1, 2))
    for i, y in enumerate(rows):
        xs = list(range(w)) if i % 2 == 0 else list(range(w - 1, -1, -1))
        path += [(y, x) for x in xs]
        if i + 1 < len(rows):
            path.append((y + 1, xs[-1]))
    return path


def corridor_wrap(d):
    """(d, 48, 64), the corridor in the middle slice: 1 559 voxels of value 10 between walls of 20, marker 1 on its first voxel.
    Marker 2 sits on its last voxel, which has value 11: with both ends at 10 the two fronts would meet after 780 generations;
    this way level 10 is flooded from one end alone, 1 558 generations, and marker 2 keeps only what touches it."""
    path = serpentine(48, 64)
    zc = d // 2
    img = np.full((d, 48, 64), WALL, np.uint16)
    for y, x in path:
        img[zc, y, x] = CORRIDOR
    mk = np.zeros(img.shape, np.int16)
    mk[(zc,) + path[0]] = 1
    mk[(zc,) + path[-1]] = 2
    img[(zc,) + path[-1]] = CORRIDOR + 1
    return img, mk


def corridor_basins():
    """(10, 48, 64), the corridor of corridor_wrap in slice 7, with four pits of value 5 (drained voxels of level 10):
      path[6..7]           reached in the same generation by the front of marker 1 (rank 0) from path[5] and by the front of
                           path[13] (rank 1: value 10, generation 0 through the voxel of value 8 under it that marker 3 holds)
      (7..8, 15..16, 15..16) without (7, 15, *): six voxels in six of the eight tiles that meet at (8, 16, 16)
      (6, 30, 20..23)      under four consecutive corridor voxels: touched again in the three generations after its stamp
      (9, 20..39, 30..49) and the shaft (8, 36, 40) above the corridor: 401 voxels, more than SK_SOLO_MAX
    Every relay has the level's 413 drained voxels to look at: it leaves the solo stretch, and the ticket carries the count."""
    path = serpentine(48, 64)
    img = np.full((10, 48, 64), WALL, np.uint16)
    for y, x in path:
        img[7, y, x] = CORRIDOR
    mk = np.zeros(img.shape, np.int16)
    mk[(7,) + path[0]] = 1
    mk[(7,) + path[-1]] = 2
    img[(7,) + path[-1]] = CORRIDOR + 1
    y13, x13 = path[13]
    img[6, y13, x13], mk[6, y13, x13] = 8, 3
    for y, x in path[6:8]:
        img[7, y, x] = PIT
    img[7, 16, 15:17] = PIT
    img[8, 15:17, 15:17] = PIT
    img[6, 30, 20:24] = PIT
    img[9, 20:40, 30:50] = PIT
    img[8, 36, 40] = PIT
    return img, mk


def lattice(shape=(24, 48, 48), one_label=False):
    """a flat volume, markers on (3 i, 3 j, 3 k) with labels cycling 1 .. 3 (one_label: all 1): with 26 neighbours every marker
    appends its 26 neighbours in the level's first round and nobody else offers them"""
    img = np.zeros(shape, np.uint16)
    mk = np.zeros(shape, np.int16)
    i, j, k = np.meshgrid(*[np.arange(0, s, 3) for s in shape], indexing="ij")
    mk[i, j, k] = 1 if one_label else (i // 3 + j // 3 + k // 3) % 3 + 1
    return img, mk


def _pierce(shape):
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    return ((3 * z + y) % 4 == 1) & ((x + 2 * z) % 5 == 2)


def tile_pierced(shape, marks):
    """a plateau of value 3 pierced by voxels of value 7; `marks` = ((z, y, x), label): label l sits on a voxel of value l - 1, so
    the plateau's generation 0 is what touches the markers -- on tile faces and corners where the markers are"""
    img = np.where(_pierce(shape), 7, 3).astype(np.uint16)
    mk = np.zeros(shape, np.int16)
    for at, l in marks:
        mk[at], img[at] = l, l - 1
    return img, mk


def tile_halo():
    """(9, 17, 33) of value 7 with a U of value 2 in slice 3: arms y = 2 and y = 5 over x = 10 .. 17, joined at x = 17.  Inside
    the tile x < 16 the arms are two parts that meet only through the next tile, whose first column is this tile's halo."""
    img = np.full((9, 17, 33), 7, np.uint16)
    img[3, 2, 10:18] = img[3, 5, 10:18] = img[3, 2:6, 17] = 2
    mk = np.zeros(img.shape, np.int16)
    mk[3, 2, 10] = 1
    mk[8, 16, 32], img[8, 16, 32] = 2, 6
    return img, mk


def tile_face_plane(axis, high):
    """(17, 33, 33): a plateau of value 3 whose generation 0 is one whole plane on a tile face and nothing else -- the plane at
    coordinate 8 | 16 | 16 of `axis` (the first of its tile; the plateau is everything below it) or, `high`, at 7 | 15 | 15 (the
    last of its tile; the plateau is everything above).  The other side has value 2 and the markers (values 0 and 1).  The tile
    across the face holds no generation 0 of its own and no voxel of the plane ever changes: only k_sk_mark_tiles wakes it."""
    shape = (17, 33, 33)
    face = (TZ, TY, TX)[axis] - (1 if high else 0)
    at = np.indices(shape)[axis]
    img = np.where((at >= face) if high else (at <= face), 3, 2).astype(np.uint16)
    mk = np.zeros(shape, np.int16)
    lowside = [4, 9, 9]
    lowside[axis] = (face - 3) if high else (face + 3)
    a, b = list(lowside), list(lowside)
    a[(axis + 1) % 3] -= 3
    b[(axis + 1) % 3] += 4
    mk[tuple(a)], img[tuple(a)] = 1, 0
    mk[tuple(b)], img[tuple(b)] = 2, 1
    return img, mk


def gen0_switch(k):
    """(8, 64, 64): level 1 has exactly k generation-0 voxels (k - 3 markers of label 1 and the three neighbours of marker 2,
    which sits on the last voxel with value 0) and 32 763 voxels; four voxels of value 2 are a level above it"""
    img = np.ones((8, 64, 64), np.uint16)
    mk = np.zeros(img.shape, np.int16)
    mk.ravel()[:k - 3] = 1
    mk[7, 63, 63], img[7, 63, 63] = 2, 0
    img[4, 32, 30:34] = 2
    return img, mk


def total_switch(n5):
    """(8, 64, 66): exactly n5 voxels of value 5 (the block x < 64 without the two markers, then voxels of the column x = 64 in
    raster order), the rest 9; marker 1 on (0, 0, 0) with value 0, marker 2 on (7, 63, 63) with value 1"""
    img = np.full((8, 64, 66), 9, np.uint16)
    img[:, :, :64] = 5
    mk = np.zeros(img.shape, np.int16)
    mk[0, 0, 0], img[0, 0, 0] = 1, 0
    mk[7, 63, 63], img[7, 63, 63] = 2, 1
    extra = n5 - int((img == 5).sum())
    assert 0 <= extra <= 512
    col = img[:, :, 64].reshape(-1)
    col[:extra] = 5
    img[:, :, 64] = col.reshape(8, 64)
    return img, mk


def slice_2d():
    """a 2-D image (the GUI's slice mode), 70 x 90: blocks of 5 x 5 with random values 3 .. 15 -- dozens of small levels with
    basins -- and three markers on values 0, 1, 2"""
    rng = np.random.default_rng(3)
    img = np.kron(rng.integers(3, 16, (14, 18)), np.ones((5, 5), np.int64)).astype(np.uint16)
    mk = np.zeros(img.shape, np.int16)
    for l, at in enumerate(((2, 2), (67, 87), (35, 45))):
        mk[at], img[at] = l + 1, l
    return img, mk


def slabs_with_pits():
    """(6, 20, 256): slabs of 32 columns whose values rise from the middle towards both ends (3, 6, 9, 12) and, off the planes
    where a slab begins, 4 % pits one below the slab's value; markers on values 0 and 1 in the middle slabs.  Generation 0 has its
    lower neighbours at -x in one half and at +x in the other.  One run of small levels with few entries: with
    IVX_SK_LATE_MAX=0 (no room kept for late-part records) kind[] has room for the run's key records."""
    rng = np.random.default_rng(8)
    shape = (6, 20, 256)
    x = np.broadcast_to(np.arange(256), shape)
    step = np.where(x >= 128, (x - 128) // 32, (127 - x) // 32)
    img = (3 * step + 3).astype(np.uint16)
    pit = (rng.random(shape) < 0.04) & (x % 32 >= 1) & (x % 32 <= 30) & (step > 0)
    img[pit] -= 1
    mk = np.zeros(shape, np.int16)
    mk[0, 0, 120], img[0, 0, 120] = 1, 0
    mk[5, 19, 140], img[5, 19, 140] = 2, 1
    return img, mk


def mixed_chain(top=65534, dtype=np.uint16):
    """(13, 80, 80) whose ascending levels are: 3 and 4 (the markers and a voxel or two: a small run), 10 (slices 0 .. 10, basin-
    free, more than 1 << 16 voxels: tile-wise), 20 (slice 11, all of it generation 0 -- more than SMALL_GEN0 -- and slice 12 with
    pits of value 15: resident, with basins), 30, 40 and `top` (single voxels in slice 12: a small run)"""
    img = np.full((13, 80, 80), 10, dtype)
    img[11:] = 20
    y, x = np.meshgrid(np.arange(80), np.arange(80), indexing="ij")
    img[12][(y % 4 == 1) & (x % 4 == 2)] = 15
    img[12, 40:48, 40:48] = 15
    img[12, 10, 10], img[12, 20, 20:22], img[12, 60, 60] = 30, 40, top
    mk = np.zeros(img.shape, np.int16)
    img[0, 0, :2] = img[0, 1, 0] = 3
    img[10, 79, 78:] = 4
    mk[0, 0, 0], mk[10, 79, 79] = 1, 2
    return img, mk


def ct_like(shape, seed):
    """the recipe of test_gpu_wssk._ct_like: five Gaussian blobs and noise in Hounsfield-like units"""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    f = np.zeros(shape)
    for _ in range(5):
        c = rng.uniform(0, 1, 3) * np.array(shape)
        s = rng.uniform(8, 24)
        f += 1800 * np.exp(-(((z - c[0]) * 2) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * s * s))
    f += rng.normal(0, 25, shape) - 1000
    return np.clip(f, -1024, 3071).astype(np.int16), np.unravel_index(int(np.argmax(f)), shape)


LATE_SHAPE = (118, 203, 237)  # the fewest slices of 203 x 237 (no extent a multiple of the tile) at which the records are granted


def late_records(shape=LATE_SHAPE):
    """The GUI's input: the 3 x 3 x 3 morphological gradient of a CT-like volume windowed to level 300, width 400.  Label 1: every
    seventh (z + y + x) of the voxels whose gradient is not 0 in a box of 21 x 49 x 49 around the brightest voxel (the rim of the blob that saturates the
    window); label 2: two corner blocks, gradient 0 there."""
    vol, am = ct_like(shape, 9)
    lo, hi = 300 - 0.5 - 399 / 2, 300 - 0.5 + 399 / 2
    win = np.where(vol <= lo, 0, np.where(vol > hi, 400, ((vol - 299.5) / 399 + 0.5) * 400)).astype(np.int16).astype(np.uint16)
    img = morphological_gradient(win, size=(3, 3, 3))
    mk = np.zeros(shape, np.int16)
    blob = (slice(max(am[0] - 10, 0), am[0] + 11), slice(max(am[1] - 24, 0), am[1] + 25), slice(max(am[2] - 24, 0), am[2] + 25))
    zyx = np.indices(shape).sum(axis=0)
    mk[blob] = np.where((img[blob] != 0) & (zyx[blob] % 7 == 0), 1, 0)
    for corner in ((slice(0, 3), slice(0, 6), slice(0, 6)), (slice(-3, None), slice(-6, None), slice(-6, None))):
        mk[corner] = np.where(img[corner] == 0, 2, 0)
    return img, mk


# ---- the table ------------------------------------------------------------------------------------------------------------------
RES = {"IVX_SK_SMALL": "0", "IVX_SK_TILE_LEVEL": "0"}  # every level through the resident launch
TILE = {"IVX_SK_SMALL": "0", "IVX_SK_TILE_LEVEL": "1"}  # every basin-free level tile-wise (is_small is asked first: off)


def _v(name, base=None, **more):
    env = dict(base or {})
    env.update(more)
    return name, env


def _case(id, build, args=(), conn=1, ndim=3, envs=(), expect=None, mk_dtypes=(np.int16,), plain=True):
    return dict(id=id, build=build, args=args, conn=conn, ndim=ndim, envs=[_v("default")] + list(envs), expect=expect or {},
                mk_dtypes=mk_dtypes, plain=plain)


_A_ENVS = [_v("solo0", RES, IVX_SK_SOLO="0"), _v("solo-default", RES), _v("solo1", RES, IVX_SK_SOLO="1")]
_B_ENVS = [_v("resident", RES), _v("perwg32", RES, IVX_SK_PER_WG="32"), _v("perwg32-solo0", RES, IVX_SK_PER_WG="32", IVX_SK_SOLO="0"),
           _v("res2", RES, IVX_SK_RES_PER_CU="2")]
_C_ENVS = [_v("resident", RES)]
_D_ENVS = [_v("tile", TILE), _v("tile-cells", TILE, IVX_SK_PLANE="0")]
_E_ENVS = [_v("norecs", IVX_SK_SMALL_RECS="0")]
_REC_ENVS = [_v("recs", IVX_SK_LATE_MAX="0"), _v("norecs", IVX_SK_LATE_MAX="0", IVX_SK_SMALL_RECS="0")]
_FACES = (((7, 2, 15), 1), ((8, 12, 16), 2), ((0, 16, 32), 3), ((4, 15, 0), 1))

# expect: what the census must show (checked by check_expect, on the CPU) for the case to be on the path it is named for.
#   kinds[variant]  the kinds of the ascending levels under that variant's knobs, first letters (s, t, r)
#   the other keys are explained at check_expect
CASES = [
    # (a)
    _case("corridor-wrap-1", corridor_wrap, (1,), envs=_A_ENVS,
          expect=dict(kinds={"default": "sss", "solo0": "rrr"}, level=10, depth=1557, words_solo0=1558, stretch_default=1557, no_basins=True)),
    _case("corridor-wrap-3", corridor_wrap, (3,), envs=_A_ENVS,
          expect=dict(kinds={"default": "ssr", "solo0": "rrr"}, level=10, depth=1557, words_solo0=1558, stretch_default=1557, no_basins=True)),
    # (b)
    _case("corridor-basins", corridor_basins, envs=_B_ENVS,
          expect=dict(kinds={"default": "sssr", "resident": "rrrr"}, level=10, basin_gens=4, drained=413)),
    # (c) -- lattice-overflow is the issue's case word for word, and the one row whose tied-marker count is not 0: its 2 048
    # markers share the value 0 and their labels change 2 047 times in raster order; that the markers do not touch does not
    # matter to the count, nor to scikit-image's heap.  lattice-overflow-1 is the same lattice with one label, tied count 0.
    _case("lattice-overflow", lattice, conn=3, envs=_C_ENVS, expect=dict(kinds={"default": "r"}, level=0, overflow=True, tied=2047, no_basins=True)),
    _case("lattice-overflow-1", lattice, ((24, 48, 48), True), conn=3, envs=_C_ENVS, expect=dict(kinds={"default": "r"}, level=0, overflow=True, no_basins=True)),
    _case("lattice-twin-6", lattice, ((24, 48, 48), True), conn=1, envs=_C_ENVS, expect=dict(kinds={"default": "r"}, level=0, overflow=False, no_basins=True)),
]
for _conn in (1, 2, 3):
    # (d)
    CASES += [
        _case("tile-faces-pierced-%d" % _conn, tile_pierced, ((9, 17, 33), _FACES), conn=_conn, envs=_D_ENVS, expect=dict(kinds={"tile": "ttttt"}, no_basins=True)),
        _case("tile-faces-halo-%d" % _conn, tile_halo, conn=_conn, envs=_D_ENVS, expect=dict(kinds={"tile": "ttt"}, no_basins=True)),
        _case("tile-faces-thin-z-%d" % _conn, tile_pierced, ((1, 17, 33), (((0, 2, 15), 1), ((0, 12, 16), 2), ((0, 16, 32), 3))), conn=_conn,
              envs=_D_ENVS, expect=dict(kinds={"tile": "ttttt"}, no_basins=True)),
        _case("tile-faces-thin-y-%d" % _conn, tile_pierced, ((9, 1, 33), (((7, 0, 15), 1), ((8, 0, 20), 2), ((0, 0, 32), 3))), conn=_conn,
              envs=_D_ENVS, expect=dict(kinds={"tile": "ttttt"}, no_basins=True)),
        _case("tile-faces-thin-x-%d" % _conn, tile_pierced, ((9, 17, 1), (((7, 2, 0), 1), ((8, 12, 0), 2), ((0, 16, 0), 3))), conn=_conn,
              envs=_D_ENVS, expect=dict(kinds={"tile": "ttttt"}, no_basins=True)),
    ]
for _axis in range(3):
    for _high in (False, True):
        for _conn in (1, 3):
            CASES.append(_case("tile-faces-plane-%s%s-%d" % ("zyx"[_axis], "+" if _high else "-", _conn), tile_face_plane, (_axis, _high), conn=_conn,
                               envs=_D_ENVS, expect=dict(kinds={"tile": "tttt"}, no_basins=True, plane_gen0=(3, 17 * 33 * 33 // (17, 33, 33)[_axis]))))
CASES += [
    # (e)
    _case("small-gen0-4096", gen0_switch, (4096,), expect=dict(kinds={"default": "sss"}, level=1, gen0=4096, runs=1)),
    _case("small-gen0-4097", gen0_switch, (4097,), expect=dict(kinds={"default": "srs"}, level=1, gen0=4097, runs=2)),
    _case("small-total-32768", total_switch, (32768,), expect=dict(kinds={"default": "ssss"}, level=5, voxels=32768, runs=1)),
    _case("small-total-32769", total_switch, (32769,), expect=dict(kinds={"default": "ssrs"}, level=5, voxels=32769, runs=2)),
    _case("small-2d-4", slice_2d, ndim=2, conn=1, envs=_E_ENVS, expect=dict(all_small=True, runs=1)),
    _case("small-2d-8", slice_2d, ndim=2, conn=2, envs=_E_ENVS, expect=dict(all_small=True, runs=1)),
    _case("small-recs-6", slabs_with_pits, conn=1, envs=_REC_ENVS, expect=dict(all_small=True, runs=1, recs={"default": False, "recs": True, "norecs": False})),
    _case("small-recs-26", slabs_with_pits, conn=3, envs=_REC_ENVS, expect=dict(all_small=True, runs=1, recs={"default": False, "recs": False, "norecs": False})),
    # (f)
    _case("mixed-chain", mixed_chain, mk_dtypes=(np.int16, np.int8), expect=dict(kinds={"default": "sstrsss"}, top=65534, runs=2)),
    _case("mixed-chain-u8", mixed_chain, (254, np.uint8), mk_dtypes=(np.int16, np.int8), expect=dict(kinds={"default": "sstrsss"}, top=254, runs=2)),
]
# (g): 5.7 M voxels -- the plain reference would take minutes, so these rows are compared with the serial oracle alone (plain=False).
# The recipe's levels above the zero plateau hold a few hundred voxels each: by default they are runs of small levels, and only
# with IVX_SK_SMALL=0 ("resident") does every level take the stamping path, whose late parts the records are for
# (late_record_levels says which levels, from the cost map).
_SMALL0 = {"IVX_SK_SMALL": "0"}
LATE_CASES = [
    _case("late-records-6", late_records, conn=1, plain=False,
          envs=[_v("norecs", IVX_SK_LATE_RECS="0"), _v("resident", _SMALL0), _v("resident-norecs", _SMALL0, IVX_SK_LATE_RECS="0")]),
    _case("late-records-26", late_records, conn=3, plain=False, envs=[_v("resident", _SMALL0)]),
]
CASE_IDS = [c["id"] for c in CASES]


def build_case(case):
    """(image, markers, structure, env variants, expect)"""
    img, mk = case["build"](*case["args"])
    return img, mk, generate_binary_structure(case["ndim"], case["conn"]), case["envs"], case["expect"]


def check_expect(case, img, mk, st, cen):
    """assert that the census puts the case on the path its `expect` names"""
    ex = case["expect"]
    envs = dict(case["envs"])
    lv = {l["c"]: l for l in cen["levels"]}
    assert cen["tied"] == ex.get("tied", 0), (case["id"], cen["tied"])
    for name, want in ex.get("kinds", {}).items():
        got = "".join(k[0] for k in chain(cen, envs[name])["kinds"])
        assert got == want, (case["id"], name, got)
    if ex.get("all_small"):
        assert set(chain(cen, {})["kinds"]) == {"small"} and len(cen["levels"]) > 3
    if "runs" in ex:
        assert chain(cen, {})["small_level_runs"] == ex["runs"]
    l = lv.get(ex.get("level"))
    for key in ("depth", "gen0", "voxels", "drained"):
        if key in ex:
            assert l[key] == ex[key], (case["id"], key, l[key])
    if ex.get("no_basins"):
        assert all(not x["basin_gens"] and not x["drained"] for x in cen["levels"])
    if "basin_gens" in ex:
        assert len(l["basin_gens"]) == ex["basin_gens"] and l["drained"] > SK_SOLO_MAX
    if "words_solo0" in ex:  # every round a hand-over word: the sequence number passes PSEQ_MOD - 1
        words, longest = handover(l, 0)
        assert words == ex["words_solo0"] > PSEQ_MOD and longest == 1
    if "stretch_default" in ex:  # one solo stretch begins more generations than there are sequence numbers
        words, longest = handover(l, SK_SOLO_MAX)
        assert longest == ex["stretch_default"] > PSEQ_MOD and words == 1
    if "overflow" in ex:
        waves = first_round_wave_appends(img, mk, st, cen, ex["level"])
        assert (max(waves) > WB_CAP) == ex["overflow"], (case["id"], max(waves))
        assert l["gen0"] > SK_SOLO_MAX  # the first round is handed to several workgroups, one pass each
    if "plane_gen0" in ex:  # the level's generation 0 is the whole plane and nothing else
        assert lv[ex["plane_gen0"][0]]["gen0"] == ex["plane_gen0"][1]
    if "top" in ex:
        assert cen["levels"][-1]["c"] == ex["top"] and int(np.asarray(img).max()) == ex["top"]
    for name, want in ex.get("recs", {}).items():
        entries = sum(x["gen0"] for x in cen["levels"])  # (one run: all levels)
        assert small_records_granted(np.asarray(img).size, int(np.asarray(st).sum()) - 1, entries, envs[name]) == want, (case["id"], name)
