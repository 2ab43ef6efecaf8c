"""k_mc_emit (csrc/k_mc.hip): the triangle emit as a grid-stride loop -- workgroup b of G takes the chunks (256 triangles
each) b, b + G, b + 2G, ... of the list, stages its tables once and asks for the next chunk's descriptors in front of the
current chunk's stores.  IVX_MC_EMIT_WGS=n (read at every call) caps G, so that small surfaces reach every stage of that loop:
with G = 1, 2, 3 a workgroup sees no chunk at all (more workgroups than chunks), one, two (first and last) or more.  Unforced,
these small surfaces get one workgroup per chunk; IVX_MC_EMIT_RESIDENT_MIN=1 gives test_resident_grid_wraps the grid that
only very large surfaces get otherwise.  Every case compares the triangle soup with the C oracle array for array,
as tests/test_gpu_mc_list_stores.py does."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import synth_volume

gpu = pytest.mark.gpu

CHUNK = 256                  # triangles a workgroup emits at a time
WGS = [1, 2, 3, None]        # forced workgroup counts; None = the grid the library chooses
MARK = np.float32(-12345.5)
NOPAD = (False, False, False, 0.0, 0)  # pad_xy, pad_bottom, pad_top, pad_value, vtk_pz


def _force(monkeypatch, wgs):
    if wgs is None:
        monkeypatch.delenv("IVX_MC_EMIT_WGS", raising=False)
    else:
        monkeypatch.setenv("IVX_MC_EMIT_WGS", str(wgs))


def _isolated(nvox, value=255, dtype=np.uint8):
    """`nvox` inside voxels two apart in the middle slice of three, none on a face of the volume: each is the one inside corner
    of eight cells of its own, that is 8 triangles, so 32 voxels are exactly one chunk"""
    cols = 16
    rows = (nvox + cols - 1) // cols
    a = np.zeros((3, 2 * rows + 1, 2 * cols + 1), dtype)
    q = np.arange(nvox)
    a[1, 1 + 2 * (q // cols), 1 + 2 * (q % cols)] = value
    return a


@functools.lru_cache(maxsize=None)
def _isolated_ref(nvox, isos=(127.5,)):
    from oracle import oracle as orc
    orc.build()
    ref = orc.marching_cubes(_isolated(nvox), (1.0, 1.0, 1.0), list(isos), 0, *NOPAD)
    assert len(ref) == 8 * nvox * len(isos)
    ref.setflags(write=False)
    return ref


class _Piece:
    """a piece counted on the device, to be emitted at any capacity into a buffer of markers"""

    def __init__(self, a, isos, pads=NOPAD, spacing=(1.0, 1.0, 1.0)):
        from invesalius3_amd import _lib as L
        from invesalius3_amd.device import DeviceBuffer
        self.L, self.lib = L, L.lib()
        pad_xy, pad_bottom, pad_top, pad_value, vtk_pz = pads
        iso = list(isos) + [0.0] * (2 - len(isos))
        self.p = L.McParams(dtype=L.dtype_code(a, (L.U8, L.I16, L.U16)), pad_xy=int(pad_xy), pad_bottom=int(pad_bottom),
                            pad_top=int(pad_top), vtk_pz=int(vtk_pz), niso=len(isos), nz=a.shape[0], ny=a.shape[1], nx=a.shape[2],
                            roi_start=0, pad_value=float(pad_value), spacing=(ctypes.c_double * 3)(*spacing),
                            iso=(ctypes.c_double * 2)(*iso))
        nb = ctypes.c_size_t(0)
        L.check(self.lib.ivx_dev_mc_scratch_bytes(ctypes.byref(self.p), ctypes.byref(nb)))
        self.d_a, self.d_s = DeviceBuffer(a.nbytes), DeviceBuffer(nb.value)
        self.d_a.upload(np.ascontiguousarray(a))
        n = ctypes.c_int64(0)
        L.check(self.lib.ivx_dev_mc_count(ctypes.byref(self.p), self.d_a.ptr, self.d_s.ptr, ctypes.byref(n), None))
        self.total = n.value

    def emit(self, cap, room, shift=0, guard=64):
        """Emit at capacity `cap` into a buffer with room for `room` triangles and `guard` floats behind them, all markers,
        `shift` floats behind the buffer's start.  Returns (triangles [room, 3, 3], guard floats, floats in front)."""
        from invesalius3_amd.device import DeviceBuffer
        floats = shift + room * 9 + guard
        d_t = DeviceBuffer(floats * 4)
        d_t.upload(np.full(floats, MARK, np.float32))
        self.L.check(self.lib.ivx_dev_mc_emit(ctypes.byref(self.p), self.d_a.ptr, self.d_s.ptr, d_t.at(4 * shift),
                                               ctypes.c_int64(cap), None))
        self.L.check(self.lib.ivx_device_synchronize())
        got = d_t.download((floats,), np.float32)
        d_t.close()
        return got[shift:shift + room * 9].reshape(room, 3, 3), got[shift + room * 9:], got[:shift]

    def close(self):
        self.d_a.close()
        self.d_s.close()


def _check_emit(piece, ref, cap, shift=0):
    room = max(cap, piece.total) + 8
    got, guard, front = piece.emit(cap, room, shift)
    n = min(cap, piece.total)
    assert np.array_equal(got[:n], ref[:n]), (cap, shift)
    assert (got[n:] == MARK).all(), (cap, shift)       # at and beyond the capacity (or the count)
    assert (guard == MARK).all() and (front == MARK).all(), (cap, shift)


# ---- chunks per workgroup ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("nvox", [32, 64, 96, 128, 160, 224, 100])
def test_chunks_per_workgroup(ivxlib, monkeypatch, nvox, wgs):
    """1, 2, 3, 4, 5 and 7 whole chunks, and 3 chunks with a partial fourth (800 triangles), on 1, 2, 3 and the unforced number
    of workgroups"""
    from invesalius3_amd import surface_process as sp
    ref = _isolated_ref(nvox)
    assert len(ref) == 8 * nvox and (len(ref) % CHUNK == 0) == (nvox != 100)
    _force(monkeypatch, wgs)
    got = sp.marching_cubes(_isolated(nvox), (1.0, 1.0, 1.0), [127.5], 0, *NOPAD)
    assert got.shape == ref.shape and np.array_equal(got, ref)


# ---- capacity ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wgs", [1, 2, None])
def test_capacity(ivxlib, monkeypatch, wgs):
    """max_tris at, around and between chunk ends, equal to the count and above it: what is below the capacity is the oracle's,
    the markers at and beyond it and the guard floats behind the buffer stay"""
    nvox = 100
    ref = _isolated_ref(nvox)
    piece = _Piece(_isolated(nvox), [127.5])
    assert piece.total == len(ref) == 800
    _force(monkeypatch, wgs)
    for cap in (1, 255, 256, 257, 511, 513, piece.total, piece.total + 300):
        _check_emit(piece, ref, cap)
    piece.close()


# ---- unaligned output --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wgs", [1, 2, None])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_unaligned_output(ivxlib, monkeypatch, shift, wgs):
    """a `tris` pointer 4, 8 and 12 bytes off 16-byte alignment: every chunk takes the scalar copy-out, several per workgroup"""
    nvox = 100
    ref = _isolated_ref(nvox)
    piece = _Piece(_isolated(nvox), [127.5])
    _force(monkeypatch, wgs)
    for cap in (piece.total, 513):
        _check_emit(piece, ref, cap, shift)
    piece.close()


# ---- two iso-values ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("nvox", [36, 64])
def test_two_isos_split(ivxlib, monkeypatch, nvox, wgs):
    """voxels of 255 are inside for both iso-values, so iso 1's triangles begin at 8 * nvox: inside the second chunk (288) and on
    the boundary between the second and the third (512)"""
    from invesalius3_amd import surface_process as sp
    isos = (127.5, 60.5)
    ref = _isolated_ref(nvox, isos)
    assert (8 * nvox % CHUNK == 0) == (nvox == 64)
    assert not np.array_equal(ref[:8 * nvox], ref[8 * nvox:])  # (the two halves differ: a wrong split shows)
    _force(monkeypatch, wgs)
    got = sp.marching_cubes(_isolated(nvox), (1.0, 1.0, 1.0), list(isos), 0, *NOPAD)
    assert got.shape == ref.shape and np.array_equal(got, ref)


# ---- all kernel forms --------------------------------------------------------------------------------------------------------
def _noise(dtype):
    rng = np.random.default_rng(77)
    if dtype == np.uint8:
        return rng.integers(0, 256, (4, 12, 40)).astype(dtype), [127.5, 60.5]
    if dtype == np.int16:
        return rng.integers(-1000, 1000, (4, 12, 40)).astype(dtype), [0.5, 300.5]
    return rng.integers(0, 4000, (4, 12, 40)).astype(dtype), [2000.5, 900.5]


@functools.lru_cache(maxsize=None)
def _noise_ref(dtype, padded):
    from oracle import oracle as orc
    orc.build()
    a, isos = _noise(dtype)
    pads = (True, True, True, float(np.iinfo(dtype).min), 1) if padded else NOPAD
    ref = orc.marching_cubes(a, (0.5, 1.0, 2.0), isos, 0, *pads)
    ref.setflags(write=False)
    return ref, pads


@gpu
@pytest.mark.parametrize("wgs", [3, None])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.uint16])
def test_voxel_forms(ivxlib, monkeypatch, dtype, padded, wgs):
    """uint8, int16 and uint16 noise through the form that gathers voxels: without padding every cell is interior, with it the
    cells of the outer shell read padding (the path with a bounds test per voxel); several chunks per workgroup under 3"""
    from invesalius3_amd import surface_process as sp
    a, isos = _noise(dtype)
    ref, pads = _noise_ref(dtype, padded)
    assert len(ref) > 8 * CHUNK
    _force(monkeypatch, wgs)
    got = sp.marching_cubes(a, (0.5, 1.0, 2.0), isos, 0, *pads)
    assert got.shape == ref.shape and np.array_equal(got, ref)


def _resident_surface(img, lo, hi, seed):
    from scipy.ndimage import generate_binary_structure
    from invesalius3_amd.device import DeviceVolume
    vol = DeviceVolume(img)
    vol.threshold(lo, hi)
    vol.region_grow([seed], lo, hi, generate_binary_structure(3, 3), fill=1, select_value=254)
    got = vol.marching_cubes(from_binary=True, download=True)
    mask = np.zeros(tuple(s + 1 for s in img.shape), np.uint8)
    mask[1:, 1:, 1:] = vol.download_mask()
    vol.close()
    return got, mask


@gpu
def test_levels_form(ivxlib, oracle, monkeypatch):
    """DeviceVolume: threshold -> region growing (selects with 254) -> marching cubes from the mask's known levels, on 1, 3 and
    the unforced number of workgroups, against the oracle and against the same volume with IVX_MASK_DEFER=0"""
    from scipy.ndimage import generate_binary_structure, label
    shape = (20, 48, 128)
    assert np.prod(shape) < 64 ** 3
    img = (synth_volume(shape, seed=31) + np.random.default_rng(32).integers(-900, 900, shape)).astype(np.int16)
    lo, hi = int(np.percentile(img, 70)), 3071
    lab, ncomp = label((img >= lo) & (img <= hi), generate_binary_structure(3, 3))
    assert ncomp > 1
    z, y, x = np.argwhere(lab == np.argmax(np.bincount(lab.ravel())[1:]) + 1)[0]
    seed = (int(x), int(y), int(z))
    monkeypatch.setenv("IVX_MASK_DEFER", "0")
    plain, mask = _resident_surface(img, lo, hi, seed)
    monkeypatch.delenv("IVX_MASK_DEFER")
    assert (mask == 254).any() and (mask == 255).any()
    want = oracle.create_surface_piece(None, mask, slice(0, shape[0]), (1.0, 1.0, 1.0), 0, 0, True)
    assert len(want) > 8 * CHUNK
    assert plain.shape == want.shape and np.array_equal(plain, want)
    for wgs in (1, 3, None):
        _force(monkeypatch, wgs)
        got, mask2 = _resident_surface(img, lo, hi, seed)
        assert np.array_equal(mask2, mask)
        assert got.shape == want.shape and np.array_equal(got, want), wgs


# ---- one wrap of the unforced grid -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wrap_case():
    from oracle import oracle as orc
    orc.build()
    a = np.random.default_rng(5).integers(0, 256, (50, 64, 64)).astype(np.uint8)
    ref = orc.marching_cubes(a, (1.0, 1.0, 1.0), [127.5], 0, *NOPAD)
    ref.setflags(write=False)
    return a, ref


@gpu
@pytest.mark.parametrize("wgs", [None, 1792, 2048])
def test_resident_grid_wraps(ivxlib, monkeypatch, wgs):
    """uint8 noise with more chunks (2 431) than a chip of 256 CUs holds workgroups of this kernel at eight per CU, its most.
    Unforced, the library takes the resident grid only from 32 chunks per workgroup on (16.8 M triangles on this chip, too
    many for a test), so IVX_MC_EMIT_RESIDENT_MIN=1 moves that line down: the grid is then the one emit_grid makes of the
    runtime's occupancy answer, smaller than the chunk count, and the real stride runs.  The two forced cases are the grids
    of eight and seven workgroups per CU whatever the runtime answers."""
    from invesalius3_amd import surface_process as sp
    a, ref = _wrap_case()
    assert a.size < 100 ** 3 and 256 * 8 * CHUNK < len(ref) < 700_000
    _force(monkeypatch, wgs)
    monkeypatch.setenv("IVX_MC_EMIT_RESIDENT_MIN", "1")
    got = sp.marching_cubes(a, (1.0, 1.0, 1.0), [127.5], 0, *NOPAD)
    assert got.shape == ref.shape and np.array_equal(got, ref)
