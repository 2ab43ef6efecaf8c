"""Test infrastructure (imports nothing from the package): the pieces that put the indexed mesh of csrc/k_mci.hip and its cross-slab
stitch on the edges of their bit arithmetic -- padded rows that end at, one before and one after a 64-bit word; samples that
EQUAL the iso-value at bit 0 and bit 63 of a word with one known crossing; padding on and inside the surface; uint16; thin and
empty pieces; more point words than one scan block -- and the constants behind those edges, restated.
tests/test_mci_cases_host.py checks, without a GPU, that every case sits where it is named and that tests/_mci_ref.py agrees with
the C oracle on all of them; tests/test_gpu_mci_edges.py runs the kernels.  Every builder is seeded.

A case is a dict: array, spacing, iso_values, roi_start, pad_xy, pad_bottom, pad_top, pad_value, vtk_pz (the arguments of
`marching_cubes_indexed`, see `args_of`), `name`, `group`, and the features it is named for."""
import numpy as np

# ---- the constants, restated (test_mci_cases_host.py matches each against the source text) ----
WORD = 64                  # k_mci.hip / mc_common.h: points per word of a padded row
GRID_CAP = 16384           # k_mci.hip: workgroups of the grid-stride kernels at the most (256 lanes each)
CROSSREC_BYTES = 32        # k_mci.hip: one CrossRec (cx, cy, cz, cp) per point word
SCAN_BLOCK = 4096          # scan_u32.h: elements per workgroup of the scan (as in _surface_switch_cases.py)

WORD_EDGE_NX = (63, 64, 65, 127, 128, 129)
PADS3 = ((True, True, True), (False, False, False), (True, False, True))
# (dk, djf, di) in PADDED coordinates: where the outside neighbour of a planted on-iso sample lies
DIRECTIONS = {"-x": (0, 0, -1), "+x": (0, 0, 1), "-y": (0, -1, 0), "+y": (0, 1, 0), "-z": (-1, 0, 0), "+z": (1, 0, 0)}


def geometry(shape, pad_xy, pad_bottom, pad_top):
    """(NZ, NY, NX, WX, ws) of make_geom (mc_common.h)"""
    nz, ny, nx = shape
    pxy = int(bool(pad_xy))
    NX = nx + 2 * pxy
    return nz + int(bool(pad_bottom)) + int(bool(pad_top)), ny + 2 * pxy, NX, -(-NX // WORD), -(-nx // WORD)


def _case(group, name, array, spacing, iso_values, roi_start, pads, pad_value, vtk_pz=None, **features):
    pad_xy, pad_bottom, pad_top = (bool(p) for p in pads)
    if vtk_pz is None:
        vtk_pz = 1 if (pad_xy and pad_bottom) else 0
    NZ, NY, NX, WX, ws = geometry(array.shape, pad_xy, pad_bottom, pad_top)
    c = dict(group=group, name=name, array=array, spacing=tuple(spacing), iso_values=[float(v) for v in iso_values],
             roi_start=int(roi_start), pad_xy=pad_xy, pad_bottom=pad_bottom, pad_top=pad_top, pad_value=float(pad_value),
             vtk_pz=int(vtk_pz), NZ=NZ, NY=NY, NX=NX, WX=WX, ws=ws)
    c.update(features)
    return c


def args_of(case, iso_values=None):
    """the arguments after the array of `marching_cubes_indexed` / `oracle.marching_cubes`"""
    return (case["spacing"], list(case["iso_values"] if iso_values is None else iso_values), case["roi_start"], case["pad_xy"],
            case["pad_bottom"], case["pad_top"], case["pad_value"], case["vtk_pz"])


def _tag(pads):
    return "".join("T" if p else "F" for p in pads)


# ---- small-integer fields: every fifth sample equals an iso-value ----
def ints_cases():
    out, seen = [], set()
    spacing, isos = (1.0, 0.5, 0.25), [2.0, 3.0]

    def add(NX, pads, vtk_pz, seed):
        key = (NX, pads, vtk_pz)
        if key in seen:
            return
        seen.add(key)
        nx = NX - 2 if pads[0] else NX
        a = np.random.default_rng(seed).integers(0, 5, (3, 4, nx)).astype(np.int16)
        out.append(_case("ints", "ints_NX%d_%s_pz%d" % (NX, _tag(pads), vtk_pz), a, spacing, isos, 5, pads, -5.0, vtk_pz,
                         want_NX=NX))

    for n, NX in enumerate(WORD_EDGE_NX):
        for m, pads in enumerate(PADS3):
            add(NX, pads, 1 if (pads[0] and pads[1]) else 0, 1000 + 10 * n + m)
    n = 0
    for pxy in (False, True):
        for pb in (False, True):
            for pt in (False, True):
                for pz in (0, 1):
                    add(65, (pxy, pb, pt), pz, 2000 + n)
                    n += 1
    return out


# ---- one on-iso sample, one outside neighbour ----
PLANTED_SHAPE = (3, 3, 130)
PLANTED_X = (0, 1, 63, 64, 128, 129)      # padded x of the on-iso sample: the row's ends and both sides of the word seam
PLANTED_AT = ((1, 1), (0, 0), (2, 2))     # (plane k, padded row jf): middle, first, last


def planted_block(shape, point, direction, dtype=np.int16):
    """`shape` filled with 10, the sample at the PADDED position `point` = (k, jf, i) set to 5 (= the iso-value) and its neighbour
    in `direction` to 0; no padding, so padded row jf is source row ny - 1 - jf.  None when the neighbour does not exist."""
    nz, ny, nx = shape
    k, jf, i = point
    dk, dj, di = DIRECTIONS[direction]
    nk, nj, ni = k + dk, jf + dj, i + di
    if not (0 <= nk < nz and 0 <= nj < ny and 0 <= ni < nx):
        return None
    a = np.full(shape, 10, dtype)
    a[k, ny - 1 - jf, i] = 5
    a[nk, ny - 1 - nj, ni] = 0
    return a


def planted_cases():
    out = []
    nz, ny, nx = PLANTED_SHAPE
    for (k, jf) in PLANTED_AT:
        for i in PLANTED_X:
            for d, (dk, dj, di) in DIRECTIONS.items():
                a = planted_block(PLANTED_SHAPE, (k, jf, i), d)
                if a is None:
                    continue
                nb = (k + dk, jf + dj, i + di)
                interior = all(0 < c < n - 1 for c, n in zip(nb, PLANTED_SHAPE))  # all six neighbours of the outside sample exist
                out.append(_case("planted", "planted_k%d_j%d_x%d_%s" % (k, jf, i, d), a, (1.0, 0.5, 0.25), [5.0], 0,
                                 (False, False, False), 0.0, 0, point=(k, jf, i), direction=d, neighbour=nb, interior=interior))
    return out


def pad_cases():
    out = []
    for group, padv in (("pad_on_iso", 2.0), ("pad_inside", 3.0)):
        for nx in (62, 63):
            a = np.random.default_rng(3000 + nx).integers(0, 4, (4, 5, nx)).astype(np.uint8)
            out.append(_case(group, "%s_NX%d" % (group, nx + 2), a, (1.0, 1.0, 1.0), [2.0], 0, (True, True, True), padv,
                             want_NX=nx + 2))
    return out


def u16_cases():
    out = []
    for NX, pads in ((65, (True, True, True)), (128, (False, False, False))):
        rng = np.random.default_rng(4000 + NX)
        nx = NX - 2 if pads[0] else NX
        a = rng.integers(30000, 50000, (4, 5, nx)).astype(np.uint16)
        a[rng.random(a.shape) < 0.08] = 40000     # some samples ON the iso-value
        out.append(_case("u16", "u16_NX%d_%s" % (NX, _tag(pads)), a, (0.5, 0.75, 2.0), [40000.0], 3, pads, 0.0, want_NX=NX))
    return out


def thin_cases():
    out = []
    for shape in ((1, 1, 1), (1, 5, 70), (4, 1, 70), (4, 5, 1), (0, 5, 7), (5, 0, 7), (5, 6, 0)):
        for pads in ((True, True, True), (False, False, False)):
            a = np.random.default_rng(5000 + sum(shape)).integers(0, 5, shape).astype(np.int16)
            out.append(_case("thin", "thin_%dx%dx%d_%s" % (shape + (_tag(pads),)), a, (1.0, 0.5, 0.25), [2.0], 5, pads, -5.0,
                             empty=0 in shape))
    for v in (2, 4):  # a single sample ON the iso-value (all six crossings meet in it) and one above it
        out.append(_case("thin", "thin_single_%d_TTT" % v, np.full((1, 1, 1), v, np.int16), (1.0, 0.5, 0.25), [2.0], 5,
                         (True, True, True), -5.0, empty=False))
    return out


def past_scan_block_case():
    a = np.random.default_rng(6000).integers(0, 5, (30, 40, 200)).astype(np.int16)
    return _case("past_scan_block", "past_scan_block", a, (1.0, 0.5, 0.25), [2.0], 5, (True, True, True), -5.0)


def piece_cases():
    """every non-stitch case"""
    return ints_cases() + planted_cases() + pad_cases() + u16_cases() + thin_cases() + [past_scan_block_case()]


def by_name(name):
    for c in piece_cases():
        if c["name"] == name:
            return c
    raise KeyError(name)


# ---- the levels path: threshold + region growing on conftest.synth_volume((6, 9, dx), seed=LEVELS_SEED) ----
LEVELS_DX = (62, 63, 64, 65, 126, 127)
LEVELS_SEED = 91
LEVELS_THRESHOLD = (-500, 3071)   # the mask: 255 here
LEVELS_GROW = (-300, 3071)        # the region grown from the first voxel in this range: 254 there, across source x = 63 | 64


# ---- the cross-slab stitch: a volume cut into `world` slabs of `nz` slices ----
STITCH_PLANTED_SHAPE = (6, 5, 130)
STITCH_PLANTED_DIRS = ("-z", "+z", "-x", "+y")   # the outside neighbour below, above and in the shared plane


def _stitch(name, whole, world, nz, fill_border_holes, iso, pad_value, spacing, **features):
    assert whole.shape[0] == world * nz
    c = dict(group="stitch", name=name, whole=whole, world=world, nz=nz, fill_border_holes=bool(fill_border_holes), iso=float(iso),
             pad_value=float(pad_value), spacing=tuple(spacing))
    c.update(features)
    return c


def blob_mask(shape=(6, 20, 70)):
    """a 0 / 255 mask: two overlapping balls and a bar that crosses every slab boundary"""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    m = ((z - 2.5) * 3.0) ** 2 + (y - 9.0) ** 2 + (x - 30.0) ** 2 < 64.0
    m |= ((z - 3.5) * 3.0) ** 2 + (y - 12.0) ** 2 + (x - 61.0) ** 2 < 49.0
    m[:, 3:5, 60:68] = True
    return np.where(m, 255, 0).astype(np.uint8)


def stitch_cases():
    out = []
    for dtype in (np.int16, np.uint16):
        for NX in (64, 65, 128):
            for fbh in (True, False):
                nx = NX - 2 if fbh else NX
                a = np.random.default_rng(7000 + NX + int(fbh)).integers(0, 5, (6, 5, nx)).astype(dtype)
                out.append(_stitch("stitch_%s_NX%d_%s" % (np.dtype(dtype).name, NX, "fbh" if fbh else "raw"), a, 3, 2, fbh, 2.0,
                                   -5.0 if dtype == np.int16 else 0.0, (1.0, 0.5, 0.25), want_NX=NX))
    nz, ny, nx = STITCH_PLANTED_SHAPE
    for i in (63, 64):
        for d in STITCH_PLANTED_DIRS:
            a = planted_block(STITCH_PLANTED_SHAPE, (3, 2, i), d)
            out.append(_stitch("stitch_planted_x%d_%s" % (i, d), a, 2, 3, False, 5.0, 0.0, (1.0, 0.5, 0.25), point=(3, 2, i),
                               direction=d, want_dropped=4 if DIRECTIONS[d][0] == 0 else 0))
    out.append(_stitch("stitch_blob", blob_mask(), 3, 2, True, 127.0, 0.0, (0.5, 0.5, 2.0), blob=True))
    return out


def stitch_piece(case, rank):
    """(array, args) of rank `rank`'s piece, restating parallel.slab_layout / slab_mc_args and DeviceVolume._mc_params: the rank's
    nz slices plus the first slice of the rank above; the bottom padded on rank 0 and the top on the last rank, both only with
    fill_border_holes, which also pads x and y; roi_start = the first slice's global index; vtk_pz = pad_bottom."""
    world, nz, fbh = case["world"], case["nz"], case["fill_border_holes"]
    z0 = rank * nz
    z1 = z0 + nz + (1 if rank < world - 1 else 0)
    pb, pt = fbh and rank == 0, fbh and rank == world - 1
    return case["whole"][z0:z1], (case["spacing"], [case["iso"]], z0, fbh, pb, pt, case["pad_value"], int(pb))


def stitch_whole_args(case):
    fbh = case["fill_border_holes"]
    return (case["spacing"], [case["iso"]], 0, fbh, fbh, fbh, case["pad_value"], int(fbh))
