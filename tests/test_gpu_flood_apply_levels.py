"""`mask[reached] = select` written from the bit planes alone (k_flood_apply_levels16 in csrc/k_flood.hip,
ivx_dev_flood_apply_levels): after a fused threshold the mask is 255 * inside plane byte for byte, so a touched 16-voxel chunk
is a function of its reached bits and its inside bits and the mask is not read.  The kernel on planes of every chunk kind, then
DeviceVolume's region growing -- which takes it exactly while that knowledge holds -- against numpy and scipy.ndimage.label."""
import ctypes

import numpy as np
import pytest
from scipy.ndimage import generate_binary_structure, label

pytestmark = pytest.mark.gpu
S26 = generate_binary_structure(3, 3).astype(np.uint8)
SHAPES = [(20, 48, 128), (5, 33, 64)]
LO, HI = 750, 3071  # (8 % of the noise is in range: below the 26-neighbour percolation threshold, many components)


def _plane(bits):
    """the bit plane of a (dz, dy, dx) bool volume with dx % 64 == 0: bit x & 63 of word (z * dy + y) * (dx / 64) + x / 64"""
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1)


def _image(shape):
    """noise whose in-range voxels form many small 26-connected components, a solid block that
    is reached as whole chunks, an empty band of rows, and in that band a line from the block with a lone in-range voxel eight
    voxels beside it: a chunk with reached bits AND an inside bit that is not reached"""
    dz, dy, dx = shape
    img = np.random.default_rng(dz).integers(-900, 900, shape).astype(np.int16)
    img[:, dy - 6:, :] = -1000
    img[1:4, 4:12, 16:48] = 1000
    img[2, 12:dy - 2, 20] = 1000
    img[2, dy - 3, 28] = 1000
    return img, (2, 6, 20)  # seed (z, y, x) inside the block


def _region(img, lo, hi, seed_zyx):
    inr = (img >= lo) & (img <= hi)
    lab, _ = label(inr, S26)
    assert lab[seed_zyx] > 0
    return inr, lab == lab[seed_zyx]


def _soup(oracle, mask):
    return oracle.marching_cubes(mask, (1.0, 1.0, 1.0), [127.0], 0, True, True, True, 0.0, 1)


def _xyz(seed_zyx):
    return [tuple(int(v) for v in seed_zyx[::-1])]


# ---- the kernel, on planes made by hand ------------------------------------------------------------------------------------
@pytest.mark.parametrize("v_in,v_sel", [(255, 254), (255, 100), (200, 0)])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_on_every_chunk_kind(ivxlib, shape, v_in, v_sel):
    """a third of the chunks without a reached bit, a third fully reached, a third with random bits; the inside plane is random
    and independent, so reached bits lie inside and outside it.  The mask holds a marker byte everywhere: a chunk without a
    reached bit keeps it (nothing is written), a chunk with one comes out as v_sel / v_in / 0 from the two planes alone."""
    from invesalius3_amd.device import DeviceBuffer
    L, lib = ivxlib, ivxlib.lib()
    dz, dy, dx = shape
    rng = np.random.default_rng(dx + v_sel)
    n = dz * dy * dx
    kind = rng.integers(0, 3, n // 16)
    reached = np.where(kind[:, None] == 0, False, np.where(kind[:, None] == 1, True, rng.random((n // 16, 16)) < 0.4))
    kind[-1] = 2
    reached[-1] = [True] + [False] * 14 + [True]  # (the very last chunk, first and last bit)
    inside = rng.random((n // 16, 16)) < 0.5
    touched = reached.any(axis=1)
    assert (~touched).any() and reached.all(axis=1).any() and (touched & ~reached.all(axis=1)).any()
    assert (reached & ~inside).any() and (touched[:, None] & inside & ~reached).any()
    marker = 7
    want = np.where(touched[:, None], np.where(reached, v_sel, np.where(inside, v_in, 0)), marker).astype(np.uint8).reshape(shape)
    d_r, d_i, d_m = DeviceBuffer(n // 8), DeviceBuffer(n // 8), DeviceBuffer(n)
    d_r.upload(_plane(reached))
    d_i.upload(_plane(inside))
    d_m.upload(np.full(shape, marker, np.uint8))
    plan = L.FloodPlan(dz, dy, dx, dx // 64, 0)
    L.check(lib.ivx_dev_flood_apply_levels(ctypes.byref(plan), d_r.ptr, d_i.ptr, d_m.ptr, v_in, v_sel, None), "flood_apply_levels")
    L.check(lib.ivx_device_synchronize())
    assert np.array_equal(d_m.download(shape, np.uint8), want)
    # the same bytes as the kernel that reads the mask, when the mask is what the planes say
    start = np.where(inside, v_in, 0).astype(np.uint8).reshape(shape)
    d_m.upload(start)
    L.check(lib.ivx_dev_flood_apply(ctypes.byref(plan), d_r.ptr, L.U8, d_m.ptr, ctypes.c_double(v_sel), None))
    L.check(lib.ivx_device_synchronize())
    old = d_m.download(shape, np.uint8)
    d_m.upload(start)
    L.check(lib.ivx_dev_flood_apply_levels(ctypes.byref(plan), d_r.ptr, d_i.ptr, d_m.ptr, v_in, v_sel, None), "flood_apply_levels")
    L.check(lib.ivx_device_synchronize())
    assert np.array_equal(d_m.download(shape, np.uint8), old)
    for d in (d_r, d_i, d_m):
        d.close()


def test_rows_that_are_not_whole_words_are_refused(ivxlib):
    from invesalius3_amd.device import DeviceBuffer
    L, lib = ivxlib, ivxlib.lib()
    d = DeviceBuffer(4096)
    plan = L.FloodPlan(2, 4, 50, 1, 0)
    with pytest.raises(TypeError, match="whole 64-voxel words"):
        L.check(lib.ivx_dev_flood_apply_levels(ctypes.byref(plan), d.ptr, d.ptr, d.ptr, 255, 254, None), "flood_apply_levels")
    d.close()


# ---- DeviceVolume ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_chunk_cases_through_region_growing(ivxlib, oracle, shape):
    """fused threshold, then a growing with the same thresholds: fully reached, partly reached and untouched chunks, and a
    partly reached chunk that holds an inside voxel of another component (it stays 255)"""
    from invesalius3_amd.device import DeviceVolume
    img, seed = _image(shape)
    inr, reg = _region(img, LO, HI, seed)
    r16, o16 = reg.reshape(-1, 16), (inr & ~reg).reshape(-1, 16)
    assert r16.all(axis=1).any() and (r16.any(axis=1) & ~r16.all(axis=1)).any() and (~r16.any(axis=1)).any()
    assert (r16.any(axis=1) & o16.any(axis=1)).any() and (~r16.any(axis=1) & o16.any(axis=1)).any()
    want = np.where(inr, 255, 0).astype(np.uint8)
    want[reg] = 254
    vol = DeviceVolume(img)
    vol.zero_out_mask()
    vol.threshold(LO, HI)
    assert vol._mask_levels == (255, None) and vol._mbits_valid  # (what the new kernel is taken on)
    vol.region_grow(_xyz(seed), LO, HI, S26, fill=1, select_value=254)
    assert vol._mask_levels == (255, 254)
    assert np.array_equal(vol.download_mask(), want)
    assert np.array_equal(vol.download_out_mask(), reg.astype(np.uint8))
    assert np.array_equal(vol.marching_cubes(download=True), _soup(oracle, want))
    vol.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_generic_thresholds_reach_outside_the_inside_plane(ivxlib, oracle, shape):
    """a click whose thresholds are wider than the mask's: reached voxels that are 0 in the mask become 254 as well"""
    from invesalius3_amd.device import DeviceVolume
    img, seed = _image(shape)
    inr, _ = _region(img, LO, HI, seed)
    _, reg = _region(img, LO - 250, HI, seed)
    assert (reg & ~inr).any() and (inr & ~reg).any()
    want = np.where(inr, 255, 0).astype(np.uint8)
    want[reg] = 254
    vol = DeviceVolume(img)
    vol.zero_out_mask()
    vol.threshold(LO, HI)
    vol.region_grow(_xyz(seed), LO - 250, HI, S26, fill=1, select_value=254)
    assert np.array_equal(vol.download_mask(), want)
    assert np.array_equal(vol.marching_cubes(download=True), _soup(oracle, want))
    vol.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_select_value_below_the_iso_value(ivxlib, oracle, shape):
    """select_value = 100: the selected voxels leave the surface, the inside plane is kept in step (ivx_dev_bits_combine) and
    the surface afterwards is the oracle's"""
    from invesalius3_amd.device import DeviceVolume
    img, seed = _image(shape)
    inr, reg = _region(img, LO, HI, seed)
    want = np.where(inr, 255, 0).astype(np.uint8)
    want[reg] = 100
    vol = DeviceVolume(img)
    vol.zero_out_mask()
    vol.threshold(LO, HI)
    vol.region_grow(_xyz(seed), LO, HI, S26, fill=1, select_value=100)
    assert vol._mbits_valid and vol._mask_levels is None
    assert np.array_equal(vol.download_mask(), want)
    soup = _soup(oracle, want)
    assert len(soup) > 0
    assert np.array_equal(vol.marching_cubes(download=True), soup)
    vol.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_after_the_note_is_gone_the_old_kernel_runs(ivxlib, oracle, shape):
    """threshold(preserve=True) keeps the 254s of the step before and an upload puts foreign bytes into the mask: either way
    the mask is no longer 255 * plane, the note is None, and `mask[reached] = select` blends into the bytes that are there"""
    from invesalius3_amd.device import DeviceVolume
    img, seed = _image(shape)
    inr, reg = _region(img, LO, HI, seed)
    vol = DeviceVolume(img)
    vol.zero_out_mask()
    vol.threshold(LO, HI)
    vol.region_grow(_xyz(seed), LO, HI, S26, fill=1, select_value=254)
    # 1. preserve: 254 stays where the new range has nothing, everything else is thresholded anew
    lo2 = LO + 100
    inr2 = (img >= lo2) & (img <= HI)
    lab2, _ = label(inr2, S26)
    others = np.argwhere(inr2 & ~reg)
    seed2 = tuple(int(v) for v in others[len(others) // 2])  # a voxel of the new range outside the first region
    reg2 = lab2 == lab2[seed2]
    want = np.where(inr2, 255, 0).astype(np.uint8)
    want[reg] = 254
    assert (reg & ~inr2).any()
    vol.zero_out_mask()
    vol.threshold(lo2, HI, preserve=True)
    assert vol._mask_levels is None
    vol.region_grow(_xyz(seed2), lo2, HI, S26, fill=1, select_value=253)
    want[reg2] = 253
    assert np.array_equal(vol.download_mask(), want)
    # 2. an edit from outside after a fused threshold
    vol.threshold(LO, HI)
    assert vol._mask_levels == (255, None)
    custom = np.where(inr, 255, 0).astype(np.uint8)
    custom[::2, ::3, ::5] = 7
    vol.mask.upload(custom)
    assert vol._mask_levels is None and not vol._mbits_valid
    vol.zero_out_mask()
    vol.region_grow(_xyz(seed), LO, HI, S26, fill=1, select_value=254)
    custom[reg] = 254
    assert np.array_equal(vol.download_mask(), custom)
    assert np.array_equal(vol.marching_cubes(download=True), _soup(oracle, custom))
    vol.close()
