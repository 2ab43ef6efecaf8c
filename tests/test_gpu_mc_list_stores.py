"""k_mc_list (csrc/k_mc.hip): the cell-parallel triangle list -- one active cell per lane in chunks of C cells, each cell's
descriptors stored by its lane at the place a block scan of the triangle counts gives it, and clipped per ENTRY at the caller's
capacity.  Every GPU case compares the triangle soup with the C oracle array for array, as tests/test_gpu_mc_front_end.py does; a
numpy restatement of the active-cell masks asserts that the block shapes a case is meant to reach do occur."""
import ctypes

import numpy as np
import pytest

from conftest import synth_volume

gpu = pytest.mark.gpu

C = 256        # cells per chunk: MCL_CHUNK in csrc/k_mc.hip (one cell per lane of a workgroup)
CELLS = 2048   # cell records a workgroup holds at a time: MCL_CELLS in csrc/k_mc.hip (a block with more takes several rounds)


def _cmp(got, ref):
    assert got.shape == ref.shape
    assert np.array_equal(got, ref)


def _grid(shape, pxy, pb, pt):
    """(NZ, NY, NX, WC) of the padded point grid, as make_geom in csrc/k_mc.hip (and _grid in test_gpu_mc_front_end.py)"""
    nz, ny, nx = shape
    NZ, NY, NX = nz + int(pb) + int(pt), ny + 2 * int(pxy), nx + 2 * int(pxy)
    return NZ, NY, NX, (NX - 1 + 63) // 64


def _word_cells(a, iso, pxy=False, pb=False, pt=False, pad_value=0.0):
    """(active cells per cell word, existing cells per cell word), words in the kernels' order: slice k, cell row j of the
    Y-FLIPPED padded grid, word w of the row"""
    NZ, NY, NX, WC = _grid(a.shape, pxy, pb, pt)
    inside = np.full((NZ, NY, NX), bool(pad_value >= iso))
    p, b = int(pxy), int(pb)
    inside[b:b + a.shape[0], p:p + a.shape[1], p:p + a.shape[2]] = a.astype(np.float64) >= iso
    inside = inside[:, ::-1, :]
    n = np.zeros((NZ - 1, NY - 1, NX - 1), np.int32)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                n += inside[dz:NZ - 1 + dz, dy:NY - 1 + dy, dx:NX - 1 + dx]
    act = np.zeros((NZ - 1, NY - 1, WC * 64), bool)
    act[:, :, :NX - 1] = (n > 0) & (n < 8)
    exist = np.zeros((NZ - 1, NY - 1, WC * 64), bool)
    exist[:, :, :NX - 1] = True
    return act.reshape(-1, 64).sum(axis=1), exist.reshape(-1, 64).sum(axis=1)


def _block_cells(per_word):
    """active cells per block of 256 consecutive cell words (the last block may be partial), as _nblocks counts them"""
    pad = (-len(per_word)) % 256
    return np.concatenate([per_word, np.zeros(pad, per_word.dtype)]).reshape(-1, 256).sum(axis=1)


def _args(isos, spacing=(1.0, 1.0, 1.0)):
    return (spacing, list(isos), 0, False, False, False, 0.0, 0)


# ---- dense blocks ------------------------------------------------------------------------------------------------------------
def _dense(shape):
    return np.random.default_rng(shape[2]).integers(0, 256, shape).astype(np.uint8)


@gpu
@pytest.mark.parametrize("isos", [[127.5], [127.5, 60.5]])
@pytest.mark.parametrize("shape", [(3, 20, 130), (4, 40, 257)])
def test_dense_blocks(ivxlib, oracle, shape, isos):
    """uint8 noise without padding: nearly every cell is active, so a block holds many chunks (and more cells than the workgroup
    keeps records of at a time) and words with all 64 cells active occur.  With two iso-values the second list pass starts wherever the first one's triangles end."""
    from invesalius3_amd import surface_process as sp
    a = _dense(shape)
    for iso in isos:
        act, exist = _word_cells(a, iso)
        assert _block_cells(act).max() > 4 * C and _block_cells(act).max() > CELLS
        assert ((act == exist) & (exist > 0)).any()  # a word with every cell it has active ...
    assert (_word_cells(a, isos[0])[0] == 64).any()    # ... and, for the first iso-value, one with all 64
    ref = oracle.marching_cubes(a, *_args(isos))
    assert len(ref) > 0
    _cmp(sp.marching_cubes(a, *_args(isos)), ref)


# ---- chunk edges -------------------------------------------------------------------------------------------------------------
def _rows_volume(ncells):
    """Two slices of rows of five voxels (four cells = one cell word per row), no padding, with exactly `ncells` active cells, all
    in one block: m rows 0 1 0 1 0 (every cell between two of them, and between the last and a flat row, is active: 4 m cells),
    two flat rows, and a last row whose r = ncells % 4 leading cells see a voxel."""
    m, r = divmod(ncells, 4)
    a = np.zeros((2, m + 3, 5), np.uint8)
    a[:, :m, 1::2] = 255
    a[:, m + 2, :] = np.array([[0, 0, 0, 0, 0], [255, 0, 0, 0, 0], [0, 255, 0, 0, 0], [255, 0, 255, 0, 0]], np.uint8)[r]
    return a


@gpu
@pytest.mark.parametrize("ncells", [C - 1, C, C + 1, 2 * C, 2 * C + 1])
def test_chunk_edges(ivxlib, oracle, ncells):
    """a block with exactly C - 1, C, C + 1, 2 C and 2 C + 1 active cells: the last chunk is one cell short of full, full, or a
    single cell"""
    from invesalius3_amd import surface_process as sp
    a = _rows_volume(ncells)
    act, _ = _word_cells(a, 127.5)
    assert len(act) <= 256 and _block_cells(act).tolist() == [ncells]
    ref = oracle.marching_cubes(a, *_args([127.5], (0.5, 1.0, 2.0)))
    assert len(ref) >= ncells
    _cmp(sp.marching_cubes(a, *_args([127.5], (0.5, 1.0, 2.0))), ref)


# ---- sparse blocks -----------------------------------------------------------------------------------------------------------
def _sparse_cases():
    lone = np.zeros((3, 5, 130), np.uint8)       # rows of three cell words (64 + 64 + 1 cells)
    lone[1, 2, 64] = 255                         # cells 63 and 64 of four cell rows: the last cell of a word and the next one's first
    cube = np.zeros((3, 200, 9), np.uint8)       # one cell word per row, 199 rows per slice: word 256 is row 57 of slice 1
    cube[1, 138:146, 2:6] = 255
    last = np.zeros((3, 200, 9), np.uint8)
    last[2, 10, 4] = 255                         # top slice, low source row = high cell row: words of the last block only
    return {"lone": lone, "cube": cube, "last": last}


@gpu
@pytest.mark.parametrize("name", ["lone", "cube", "last"])
def test_sparse_blocks(ivxlib, oracle, name):
    """a lone inside voxel whose cells lie in two words of a row; a small cube whose cells straddle the boundary between two
    blocks; a volume whose only active block is the last, partial one"""
    from invesalius3_amd import surface_process as sp
    a = _sparse_cases()[name]
    act, _ = _word_cells(a, 127.5)
    blocks = _block_cells(act)
    if name == "lone":
        assert act.sum() == 8 and (act > 0).sum() == 8 and act.reshape(-1, 3)[:, 2].sum() == 0
        assert (act.reshape(-1, 3)[:, 0] > 0).any() and (act.reshape(-1, 3)[:, 1] > 0).any()
    elif name == "cube":
        assert len(blocks) == 2 and act[255] > 0 and act[256] > 0
    else:
        assert len(act) % 256 != 0 and blocks[:-1].sum() == 0 and blocks[-1] > 0
    ref = oracle.marching_cubes(a, *_args([127.5]))
    assert len(ref) > 0
    _cmp(sp.marching_cubes(a, *_args([127.5])), ref)


# ---- odd start ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [(3, 20, 130), (4, 40, 257)])
def test_odd_start(ivxlib, oracle, shape):
    """The dense volume with its first two cell rows flattened, without and with one inside voxel at the first corner of the
    grid (source row ny - 1: the rows are flipped): that is one cell and one triangle in front of everything else, so every later
    list position moves by one entry (an 8-byte entry at an odd position is not 16-byte aligned)."""
    from invesalius3_amd import surface_process as sp
    a = _dense(shape)
    a[:, -3:, :] = 0
    counts = []
    for first in (0, 255):
        a[0, -1, 0] = first
        act, _ = _word_cells(a, 127.5)
        assert act[0] == (1 if first else 0) and _block_cells(act).max() > 4 * C
        ref = oracle.marching_cubes(a, *_args([127.5]))
        counts.append(len(ref))
        _cmp(sp.marching_cubes(a, *_args([127.5])), ref)
    assert counts[1] == counts[0] + 1


# ---- capacity ----------------------------------------------------------------------------------------------------------------
@gpu
def test_capacity_is_clipped_per_entry(ivxlib, oracle):
    """ivx_dev_mc_count, then ivx_dev_mc_emit with max_tris below the count: the first max_tris triangles are the oracle's and
    nothing behind them is touched -- also when max_tris falls inside a cell word's or a cell's triangles."""
    from invesalius3_amd import _lib as L
    from invesalius3_amd.device import DeviceBuffer
    lib = L.lib()
    a = np.random.default_rng(4242).integers(-1000, 1000, (3, 12, 70)).astype(np.int16)
    ref = oracle.marching_cubes(a, (1.0, 1.0, 1.0), [0.5], 0, True, True, True, -32768.0, 1)
    total = len(ref)
    assert total > 600
    p = L.McParams(dtype=L.I16, pad_xy=1, pad_bottom=1, pad_top=1, vtk_pz=1, niso=1, nz=a.shape[0], ny=a.shape[1], nx=a.shape[2],
                   roi_start=0, pad_value=-32768.0, spacing=(ctypes.c_double * 3)(1, 1, 1), iso=(ctypes.c_double * 2)(0.5, 0))
    nb = ctypes.c_size_t(0)
    L.check(lib.ivx_dev_mc_scratch_bytes(ctypes.byref(p), ctypes.byref(nb)))
    d_a, d_s, d_t = DeviceBuffer(a.nbytes), DeviceBuffer(nb.value), DeviceBuffer((total + 8) * 36)
    d_a.upload(a)
    n = ctypes.c_int64(0)
    L.check(lib.ivx_dev_mc_count(ctypes.byref(p), d_a.ptr, d_s.ptr, ctypes.byref(n), None))
    assert n.value == total
    marker = np.full((total + 8, 3, 3), -12345.5, np.float32)
    for cap in (1, 255, 256, 257, total - 1, total):
        d_t.upload(marker)
        L.check(lib.ivx_dev_mc_emit(ctypes.byref(p), d_a.ptr, d_s.ptr, d_t.ptr, ctypes.c_int64(cap), None))
        L.check(lib.ivx_device_synchronize())
        got = d_t.download(marker.shape, np.float32)
        assert np.array_equal(got[:cap], ref[:cap]), cap
        assert np.array_equal(got[cap:], marker[cap:]), cap
    for d in (d_a, d_s, d_t):
        d.close()


# ---- the resident pipeline ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("prefetch", [False, True])
def test_resident_surface_grows_and_settles(ivxlib, oracle, prefetch):
    """DeviceVolume: threshold -> region growing (selects with 254) -> marching cubes of the mask.  First with a high lower
    threshold, then with one whose surface has more than 1.25 times the triangles (it outgrows the buffer and is emitted again
    with the count as capacity), then once more in steady state (capacity above the count).  With `prefetch`, count and list are
    queued on the second stream before the region growing (DeviceVolume.surface_prefetch)."""
    from scipy.ndimage import generate_binary_structure, label
    from invesalius3_amd.device import DeviceVolume
    shape = (20, 48, 128)
    img = (synth_volume(shape, seed=31) + np.random.default_rng(32).integers(-900, 900, shape)).astype(np.int16)
    s26 = generate_binary_structure(3, 3)
    vol = DeviceVolume(img)
    sizes, queued = [], []
    for pct in (93, 70, 70):
        lo, hi = int(np.percentile(img, pct)), 3071
        lab, ncomp = label((img >= lo) & (img <= hi), s26)
        assert ncomp > 1
        z, y, x = np.argwhere(lab == np.argmax(np.bincount(lab.ravel())[1:]) + 1)[0]
        vol.threshold(lo, hi)
        if prefetch:
            queued.append(vol.surface_prefetch())
        vol.region_grow([(int(x), int(y), int(z))], lo, hi, s26, fill=1, select_value=254)
        got = vol.marching_cubes(from_binary=True, download=True)
        mask = np.zeros(tuple(s + 1 for s in shape), np.uint8)
        mask[1:, 1:, 1:] = vol.download_mask()
        assert (mask == 254).any() and (mask == 255).any()
        want = oracle.create_surface_piece(None, mask, slice(0, shape[0]), (1.0, 1.0, 1.0), 0, 0, True)
        _cmp(got, want)
        sizes.append(len(want))
    assert sizes[0] > 0 and sizes[1] > (int(sizes[0] * 36 * 1.25) + 4096) // 36  # (the buffer DeviceVolume sized from the first count)
    if prefetch:
        assert queued == [False, True, True]  # (the first call has no triangle buffer yet: nothing to size the list from)
    vol.close()
