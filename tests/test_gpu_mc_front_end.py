"""The passes in front of k_mc_emit (k_mc_count, k_mc_scan, k_mc_list in csrc/k_mc.hip): the interior form of the corner
loads, the division-free cell-word id -> (slice, row, word), the coalesced scan and the list's early exit.  Every GPU case
compares the triangle soup with the C oracle array for array, as tests/test_gpu_mc.py does."""
import ctypes

import numpy as np
import pytest

from conftest import synth_volume

gpu = pytest.mark.gpu


def _cmp(got, ref):
    assert got.shape == ref.shape
    assert np.array_equal(got, ref)


def _grid(shape, pxy, pb, pt):
    """(NZ, NY, NX, WC) of the padded point grid, as make_geom in csrc/mc_common.h"""
    nz, ny, nx = shape
    NZ, NY, NX = nz + int(pb) + int(pt), ny + 2 * int(pxy), nx + 2 * int(pxy)
    return NZ, NY, NX, (NX - 1 + 63) // 64


def _nblocks(shape, pxy, pb, pt):
    NZ, NY, NX, WC = _grid(shape, pxy, pb, pt)
    return ((NZ - 1) * (NY - 1) * WC + 255) // 256


def _wave_kinds(shape, pxy, pb, pt):
    """(#waves of 64 cell words whose four rows are all source rows, #other waves): the interior form's precondition,
    restated with numpy"""
    NZ, NY, NX, WC = _grid(shape, pxy, pb, pt)
    wid = np.arange((NZ - 1) * (NY - 1) * WC, dtype=np.int64)
    row = wid // WC
    k, j = row // (NY - 1), row % (NY - 1)
    ja, ka = (NY - 1 - j) - int(pxy), k - int(pb)
    inner = (ja - 1 >= 0) & (ja < shape[1]) & (ka >= 0) & (ka + 1 < shape[0])
    pad = (-len(inner)) % 64
    inner = np.concatenate([inner, np.ones(pad, bool)]).reshape(-1, 64).all(axis=1)
    return int(inner.sum()), int((~inner).sum())


def _shape_with_inner_waves(nz, nx, pxy, pz):
    """ny = 40, or 90 where 40 rows leave no wave of 64 words between the pad rows (rows of one or two words)"""
    for ny in (40, 90):
        if _wave_kinds((nz, ny, nx), pxy, pz, pz)[0] > 0:
            return (nz, ny, nx)
    raise AssertionError("no interior wave")


# ---- word edges ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pad_z", [True, False])
@pytest.mark.parametrize("pad_xy", [True, False])
@pytest.mark.parametrize("nx", [62, 63, 64, 65, 127, 128, 129, 191])
def test_word_edges_interior_and_boundary_waves(ivxlib, oracle, nx, pad_xy, pad_z):
    """int16 noise: every case index occurs and cell 63 of a word takes its far corners from the next word.  Rows that are and
    are not whole words, with and without the pad column in front; the shape holds waves that take the interior form and
    waves at j = 0, j = NY-2, k = 0 and k = NZ-2 that do not."""
    from invesalius3_amd import surface_process as sp
    shape = _shape_with_inner_waves(4, nx, pad_xy, pad_z)
    inner, outer = _wave_kinds(shape, pad_xy, pad_z, pad_z)
    assert inner > 0 and (outer > 0 or not (pad_xy or pad_z))
    a = np.random.default_rng(100 + nx).integers(-1000, 1000, shape).astype(np.int16)
    args = ((0.5, 0.75, 2.0), [0.5], 7, pad_xy, pad_z, pad_z, float(np.iinfo(np.int16).min), int(pad_xy and pad_z))
    ref = oracle.marching_cubes(a, *args)
    assert len(ref) > 0
    _cmp(sp.marching_cubes(a, *args), ref)


# ---- padding that counts as inside -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("isos,padv", [([-32768.0, 200.5], -32768.0), ([0.5, 300.5], 500.0)])
@pytest.mark.parametrize("nx", [63, 130])
def test_padding_inside_the_surface(ivxlib, oracle, nx, isos, padv):
    """pad_value >= iso: the pad bits are all ones (for iso -32768 everything is inside and that surface is empty; with a pad
    value of 500 both surfaces close against the padding).  The interior form must carry the pad bits of the pad COLUMNS."""
    from invesalius3_amd import surface_process as sp
    shape = _shape_with_inner_waves(5, nx, True, True)
    a = np.random.default_rng(7).integers(-1000, 1000, shape).astype(np.int16)
    for pads in ((True, True, True), (True, False, False), (False, True, True)):
        args = ((1.0, 1.0, 1.0), isos, 0, *pads, padv, int(pads[0] and pads[1]))
        ref = oracle.marching_cubes(a, *args)
        assert len(ref) > 0
        _cmp(sp.marching_cubes(a, *args), ref)


# ---- the benchmark's own path ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("env", [{}, {"IVX_MC_LEVELS": "0"}])
@pytest.mark.parametrize("shape", [(20, 48, 128), (5, 33, 64)])
def test_resident_threshold_grow_surface(ivxlib, oracle, monkeypatch, shape, env):
    """DeviceVolume: threshold (inside plane written by the same pass), 26-neighbour region growing that selects with 254,
    marching cubes of the mask -- against the oracle's surface of the downloaded mask.  Twice, so that the second surface finds
    the first one's triangle buffer."""
    from scipy.ndimage import generate_binary_structure
    from invesalius3_amd.device import DeviceVolume
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    from scipy.ndimage import label
    img = (synth_volume(shape, seed=31) + np.random.default_rng(32).integers(-900, 900, shape)).astype(np.int16)
    lo, hi = int(np.percentile(img, 75)), 3071
    lab, ncomp = label((img >= lo) & (img <= hi), generate_binary_structure(3, 3))
    assert ncomp > 1  # the seed's component becomes 254, the others stay 255
    z, y, x = np.argwhere(lab == np.argmax(np.bincount(lab.ravel())[1:]) + 1)[0]
    vol = DeviceVolume(img)
    for _ in range(2):
        vol.threshold(lo, hi)
        vol.region_grow([(int(x), int(y), int(z))], lo, hi, generate_binary_structure(3, 3), fill=1, select_value=254)
        got = vol.marching_cubes(from_binary=True, download=True)
        mask = np.zeros(tuple(s + 1 for s in shape), np.uint8)
        mask[1:, 1:, 1:] = vol.download_mask()
        assert (mask == 254).any() and (mask == 255).any()
        want = oracle.create_surface_piece(None, mask, slice(0, shape[0]), (1.0, 1.0, 1.0), 0, 0, True)
        assert len(want) > 0
        _cmp(got, want)
    vol.close()


# ---- scan lengths ----------------------------------------------------------------------------------------------------------
# number of workgroup sums per iso-value = ceil(nrows * WC / 256); rows of two voxels are one cell word each (no padding)
_SCAN_SHAPES = {1: (3, 9, 2), 63: (127, 129, 2), 64: (129, 129, 2), 65: (129, 131, 2), 1023: (342, 769, 2),
                1025: (401, 657, 2), 4097: (257, 4098, 2)}


@gpu
@pytest.mark.parametrize("nsums", sorted(_SCAN_SHAPES))
def test_scan_lengths(ivxlib, oracle, nsums):
    """1, 63, 64, 65, 1 023, 1 025 and 4 097 workgroup sums with one iso-value (a wave, a round of the scan and the guarded
    tail on either side of their edges); the two-iso surface of the same volume scans twice as many in one go."""
    from invesalius3_amd import surface_process as sp
    shape = _SCAN_SHAPES[nsums]
    assert _nblocks(shape, False, False, False) == nsums
    a = np.random.default_rng(nsums).integers(0, 256, shape).astype(np.uint8)
    for isos in ([200.5], [200.5, 40.5]):
        args = ((1.0, 1.0, 1.0), isos, 0, False, False, False, 0.0, 0)
        ref = oracle.marching_cubes(a, *args)
        assert len(ref) > 0
        _cmp(sp.marching_cubes(a, *args), ref)


@gpu
def test_scan_over_two_workgroups(ivxlib, oracle):
    """More than 16 384 workgroup sums, so k_mc_scan runs two workgroups and the second one adds up the first chunk itself.
    Rows of 8 voxels are one cell word; cell word (k * 2049 + j) belongs to sum (k * 2049 + j) / 256, and sum 16 384 begins at
    k = 2047, j = 1.  Cubes: one in the first chunk, one across k = 2047 (j = 0 .. 5, i.e. the highest source rows: y is
    flipped), one in the last rows of the last slice."""
    from invesalius3_amd import surface_process as sp
    shape = (2050, 2050, 8)
    assert _nblocks(shape, False, False, False) > 16384
    a = np.zeros(shape, np.uint8)
    a[10:14, 100:104, 2:6] = 255
    a[2045:2050, 2044:2049, 2:6] = 255
    a[2046:2050, 0:4, 2:6] = 255
    args = ((1.0, 1.0, 1.0), [127.0], 0, False, False, False, 0.0, 0)
    ref = oracle.marching_cubes(a, *args)
    assert len(ref) > 100
    _cmp(sp.marching_cubes(a, *args), ref)


# ---- the division-free split of a cell-word id (host arithmetic, no device) ------------------------------------------------
def _split(nx, ny, wid):
    from invesalius3_amd import _lib
    lib = _lib.lib()
    p = _lib.McParams(dtype=_lib.U8, pad_xy=0, pad_bottom=0, pad_top=0, vtk_pz=0, niso=1, nz=2, ny=ny, nx=nx, roi_start=0,
                      pad_value=0.0, spacing=(ctypes.c_double * 3)(1, 1, 1), iso=(ctypes.c_double * 2)(127, 0))
    wid = np.ascontiguousarray(wid, dtype=np.uint32)
    k, j, w = (np.empty(len(wid), np.uint32) for _ in range(3))
    lib.ivx_mc_split_word_ids.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 3
    lib.ivx_mc_split_word_ids.restype = ctypes.c_int
    _lib.check(lib.ivx_mc_split_word_ids(ctypes.byref(p), _lib.ptr(wid), len(wid), _lib.ptr(k), _lib.ptr(j), _lib.ptr(w)))
    return k, j, w


@pytest.mark.parametrize("wc", list(range(1, 65)) + [32768])
def test_word_id_split_is_integer_division(wc):
    """wid -> (wid / WC / (NY-1), wid / WC % (NY-1), wid % WC) for random and extreme ids below 2^32, every WC in 1 .. 64 and
    the largest one, and a spread of NY (2, powers of two and their neighbours, the largest)."""
    rng = np.random.default_rng(wc)
    nx = 64 * wc + 1 if wc > 1 else 2  # unpadded: WC = ceil((nx - 1) / 64)
    edge = np.array([0, 1, 2, wc - 1, wc, wc + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2, 2 ** 32 - 1], np.uint64)
    for ny in (2, 3, 4, 5, 8, 10, 64, 65, 66, 513, 514, 515, 1000, 4097, 32769, 65535, 65536):
        rows = np.uint64(ny - 1)
        near = (rng.integers(0, 2 ** 32 // (wc * (ny - 1)) + 1, 64).astype(np.uint64) * np.uint64(wc) * rows)  # multiples of a slice
        wid = np.concatenate([edge, rng.integers(0, 2 ** 32, 4000, dtype=np.uint64), near, near + np.uint64(1),
                              near - np.uint64(1), near + np.uint64(wc), near - np.uint64(wc)]) & np.uint64(2 ** 32 - 1)
        k, j, w = _split(nx, ny, wid)
        row = wid // np.uint64(wc)
        assert np.array_equal(w, wid % np.uint64(wc))
        assert np.array_equal(j, row % rows)
        assert np.array_equal(k, row // rows)
