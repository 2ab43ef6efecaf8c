"""The triangle count that k_mc_scan publishes itself (csrc/k_mc.hip, ivx_dev_mc_total_early): the same number as
ivx_dev_mc_total, before and after the emit, for one scan workgroup and for two, for pieces without triangles, after the
mailbox slot has gone to other messages, and for a two-iso piece (which takes the old way and sets the split).  Then
DeviceVolume.marching_cubes, which now returns while list and emit are still queued: steps queued back to back and a surface
that outgrows its buffer, against the oracle."""
import ctypes

import numpy as np
import pytest
from scipy.ndimage import generate_binary_structure, label

from conftest import synth_volume

pytestmark = pytest.mark.gpu
c64 = ctypes.c_int64
S26 = generate_binary_structure(3, 3).astype(np.uint8)
NOPAD = ((1.0, 1.0, 1.0), 0, False, False, False, 0.0, 0)  # spacing, roi_start, pad_xy, pad_bottom, pad_top, pad_value, vtk_pz


def _cmp(got, ref):
    assert got.shape == ref.shape
    assert np.array_equal(got, ref)


def _piece(L, a, isos, pad=False, pad_value=0.0):
    """(params, scratch, voxels on the device) of the piece `a`, unpadded or fully padded"""
    from invesalius3_amd.device import DeviceBuffer
    f = int(bool(pad))
    p = L.McParams(dtype=L.DT[a.dtype], pad_xy=f, pad_bottom=f, pad_top=f, vtk_pz=f, niso=len(isos), nz=a.shape[0], ny=a.shape[1],
                   nx=a.shape[2], roi_start=0, pad_value=pad_value, spacing=(ctypes.c_double * 3)(1, 1, 1),
                   iso=(ctypes.c_double * 2)(*(list(isos) + [0.0])[:2]))
    nb = ctypes.c_size_t(0)
    L.check(L.lib().ivx_dev_mc_scratch_bytes(ctypes.byref(p), ctypes.byref(nb)))
    d_a = DeviceBuffer(a.nbytes)
    if a.nbytes:
        d_a.upload(a)
    return p, DeviceBuffer(nb.value), d_a


def _early(L, p, d_s):
    n = c64(-1)
    L.check(L.lib().ivx_dev_mc_total_early(ctypes.byref(p), d_s.ptr, ctypes.byref(n), None), "mc_total_early")
    return n.value


def _total(L, p, d_s):
    n = c64(-1)
    L.check(L.lib().ivx_dev_mc_total(ctypes.byref(p), d_s.ptr, ctypes.byref(n), None), "mc_total")
    return n.value


def _three_cubes():
    a = np.zeros((2050, 2050, 8), np.uint8)  # tests/test_gpu_mc_front_end.py::test_scan_over_two_workgroups
    a[10:14, 100:104, 2:6] = 255
    a[2045:2050, 2044:2049, 2:6] = 255
    a[2046:2050, 0:4, 2:6] = 255
    return a, 127.0


def _noise(shape):
    return np.random.default_rng(shape[0]).integers(0, 256, shape).astype(np.uint8), 200.5


@pytest.mark.parametrize("make,shape", [(_noise, (3, 9, 2)), (_noise, (129, 131, 2)), (_three_cubes, None)],
                         ids=["1_sum", "65_sums", "two_scan_workgroups"])
def test_early_total_is_the_total_and_the_soup_is_the_oracles(ivxlib, oracle, make, shape):
    """queue-only count; the early total before the emit, ivx_dev_mc_total right behind it, the emit, then both again (the
    early one twice): always the oracle's count, and the emitted soup is the oracle's"""
    from invesalius3_amd.device import DeviceBuffer
    L, lib = ivxlib, ivxlib.lib()
    a, iso = make(shape) if shape else make()
    ref = oracle.marching_cubes(a, NOPAD[0], [iso], *NOPAD[1:])
    assert len(ref) > 0
    p, d_s, d_a = _piece(L, a, [iso])
    d_t = DeviceBuffer(len(ref) * 36)
    L.check(lib.ivx_dev_mc_count_async(ctypes.byref(p), d_a.ptr, d_s.ptr, None))
    assert _early(L, p, d_s) == len(ref)
    assert _total(L, p, d_s) == len(ref)
    L.check(lib.ivx_dev_mc_emit(ctypes.byref(p), d_a.ptr, d_s.ptr, d_t.ptr, c64(len(ref)), None))
    assert _early(L, p, d_s) == len(ref)
    assert _early(L, p, d_s) == len(ref)
    assert _total(L, p, d_s) == len(ref)
    assert _early(L, p, d_s) == len(ref)
    L.check(lib.ivx_device_synchronize())
    _cmp(d_t.download(ref.shape, np.float32), ref)
    # the count that returns the total itself reads the scan's word too
    n = c64(-1)
    L.check(lib.ivx_dev_mc_count(ctypes.byref(p), d_a.ptr, d_s.ptr, ctypes.byref(n), None))
    assert n.value == len(ref) == _early(L, p, d_s)
    for d in (d_s, d_a, d_t):
        d.close()


def test_pieces_without_triangles(ivxlib):
    """an all-zero volume (the scan runs and publishes 0) and an empty piece (nothing runs at all)"""
    L, lib = ivxlib, ivxlib.lib()
    for shape, pad in (((3, 9, 2), False), ((6, 20, 70), True), ((0, 6, 7), False)):
        a = np.zeros(shape, np.uint8)
        p, d_s, d_a = _piece(L, a, [127.0], pad)
        n = c64(-1)
        L.check(lib.ivx_dev_mc_count(ctypes.byref(p), d_a.ptr, d_s.ptr, ctypes.byref(n), None))
        assert n.value == 0
        L.check(lib.ivx_dev_mc_count_async(ctypes.byref(p), d_a.ptr, d_s.ptr, None))
        assert _early(L, p, d_s) == 0 and _total(L, p, d_s) == 0 and _early(L, p, d_s) == 0
        d_s.close()
        d_a.close()


def test_a_recycled_mailbox_slot_falls_back(ivxlib, oracle):
    """70 other messages go through the 64-slot mailbox between the queue-only count and the early total: the scan's word is
    gone, and the answer (now fetched the old way) is still the count -- of THIS piece, not the other one's"""
    from invesalius3_amd.device import DeviceBuffer
    L, lib, rng = ivxlib, ivxlib.lib(), np.random.default_rng(61)
    a, b = (rng.integers(0, 256, s).astype(np.uint8) for s in ((6, 20, 70), (3, 9, 2)))
    ref_a = oracle.marching_cubes(a, (1.0, 1.0, 1.0), [127.0], 0, True, True, True, 0.0, 1)
    ref_b = oracle.marching_cubes(b, NOPAD[0], [127.0], *NOPAD[1:])
    assert len(ref_a) != len(ref_b) and len(ref_b) > 0
    p_a, s_a, d_a = _piece(L, a, [127.0], True)
    p_b, s_b, d_b = _piece(L, b, [127.0])
    L.check(lib.ivx_dev_mc_count_async(ctypes.byref(p_b), d_b.ptr, s_b.ptr, None))
    L.check(lib.ivx_dev_mc_count_async(ctypes.byref(p_a), d_a.ptr, s_a.ptr, None))
    for _ in range(70):
        assert _total(L, p_b, s_b) == len(ref_b)
    assert _early(L, p_a, s_a) == len(ref_a)
    assert _early(L, p_b, s_b) == len(ref_b)
    d_t = DeviceBuffer(len(ref_a) * 36)
    L.check(lib.ivx_dev_mc_emit(ctypes.byref(p_a), d_a.ptr, s_a.ptr, d_t.ptr, c64(len(ref_a)), None))
    assert _early(L, p_a, s_a) == len(ref_a)
    L.check(lib.ivx_device_synchronize())
    _cmp(d_t.download(ref_a.shape, np.float32), ref_a)
    for d in (s_a, d_a, s_b, d_b, d_t):
        d.close()


def test_two_iso_piece_gets_total_and_split(ivxlib, oracle):
    """as tests/test_gpu_mc.py::test_indexed_calls_behind_a_queue_only_count_need_the_total, with the early form in the place of
    ivx_dev_mc_total: it returns the total of both surfaces and leaves the iso-0 / iso-1 split set, so the indexed emit works"""
    from invesalius3_amd.device import DeviceBuffer
    L, lib, rng = ivxlib, ivxlib.lib(), np.random.default_rng(52)
    isos, padv = [0.5, 300.5], float(np.iinfo(np.int16).min)
    earlier = rng.integers(-1000, 1000, (5, 12, 66)).astype(np.int16)
    a = rng.integers(-1000, 1000, (5, 12, 66)).astype(np.int16)
    soup = oracle.marching_cubes(a, (1.0, 1.0, 1.0), isos, 0, True, True, True, padv, 1)
    split = len(oracle.marching_cubes(a, (1.0, 1.0, 1.0), isos[:1], 0, True, True, True, padv, 1))
    split_earlier = len(oracle.marching_cubes(earlier, (1.0, 1.0, 1.0), isos[:1], 0, True, True, True, padv, 1))
    assert 0 < split < len(soup) and split_earlier != split
    p, d_s, d_a = _piece(L, a, isos, True, padv)
    n, nv = c64(0), c64(0)
    d_a.upload(earlier)
    L.check(lib.ivx_dev_mc_count(ctypes.byref(p), d_a.ptr, d_s.ptr, ctypes.byref(n), None))
    d_a.upload(a)
    L.check(lib.ivx_dev_mc_count_async(ctypes.byref(p), d_a.ptr, d_s.ptr, None))
    L.check(lib.ivx_dev_mc_indexed_count(ctypes.byref(p), d_a.ptr, d_s.ptr, ctypes.byref(nv), None))
    d_v, d_f = DeviceBuffer(nv.value * 12), DeviceBuffer(len(soup) * 12)
    emit = lambda: L.check(lib.ivx_dev_mc_indexed_emit(ctypes.byref(p), d_a.ptr, d_s.ptr, d_v.ptr, c64(nv.value), d_f.ptr,
                                                       c64(len(soup)), None))
    with pytest.raises(TypeError, match="ivx_dev_mc_indexed_emit must follow ivx_dev_mc_count"):
        emit()
    assert _early(L, p, d_s) == len(soup)
    nv2 = c64(0)
    L.check(lib.ivx_dev_mc_indexed_count(ctypes.byref(p), d_a.ptr, d_s.ptr, ctypes.byref(nv2), None))
    assert nv2.value == nv.value
    emit()
    L.check(lib.ivx_device_synchronize())
    verts, faces = d_v.download((nv.value, 3), np.float32), d_f.download((len(soup), 3), np.int32)
    _cmp(verts[faces], soup)
    for d in (d_s, d_a, d_v, d_f):
        d.close()


# ---- DeviceVolume: marching_cubes() returns with list and emit still queued ------------------------------------------------
SHAPES = [(20, 48, 128), (5, 33, 64)]
HI = 4000  # (above the image's maximum: the brightest voxel is a seed for every lower threshold)


def _image(shape):
    return (synth_volume(shape, seed=31) + np.random.default_rng(32).integers(-900, 900, shape)).astype(np.int16)


def _expected(oracle, img, lo, hi, seed_zyx):
    """(mask after threshold + 26-neighbour region growing that selects with 254, its surface), numpy + scipy.ndimage.label"""
    inr = (img >= lo) & (img <= hi)
    lab, _ = label(inr, S26)
    assert lab[seed_zyx] > 0
    mask = np.where(inr, 255, 0).astype(np.uint8)
    mask[lab == lab[seed_zyx]] = 254
    padded = np.zeros(tuple(s + 1 for s in img.shape), np.uint8)
    padded[1:, 1:, 1:] = mask
    return mask, oracle.create_surface_piece(None, padded, slice(0, img.shape[0]), (1.0, 1.0, 1.0), 0, 0, True)


@pytest.mark.parametrize("shape", SHAPES)
def test_three_steps_back_to_back_without_sync(ivxlib, oracle, shape):
    """threshold, grow, marching_cubes() three times with nothing in between: every step's threshold rewrites the mask and the
    inside plane while the previous step's emit may still be queued.  Each returned count is that step's; after one sync() at the
    end, soup and mask are the last step's."""
    from invesalius3_amd.device import DeviceVolume
    img = _image(shape)
    seed = tuple(int(v) for v in np.unravel_index(int(np.argmax(img)), img.shape))
    los = [int(np.percentile(img, q)) for q in (75, 65, 85)]
    want = [_expected(oracle, img, lo, HI, seed) for lo in los]
    assert len({len(w[1]) for w in want}) == 3 and all(len(w[1]) > 0 for w in want)
    vol = DeviceVolume(img)
    vol.threshold(min(los), HI)
    vol.marching_cubes()  # (gives the volume a triangle buffer with room for every step: they take the steady-state branch)
    cap = vol._tris.nbytes // 36
    assert all(len(w[1]) <= cap for w in want)
    counts = []
    for lo in los:
        vol.zero_out_mask()
        vol.threshold(lo, HI)
        vol.region_grow([seed[::-1]], lo, HI, S26, fill=1, select_value=254)
        counts.append(vol.marching_cubes(from_binary=True))
    assert counts == [len(w[1]) for w in want]
    vol.sync()
    _cmp(vol._tris.download((counts[-1], 3, 3), np.float32), want[-1][1])
    _cmp(vol.download_mask(), want[-1][0])
    vol.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_surface_outgrows_the_buffer_without_download(ivxlib, oracle, shape):
    """a small surface, then one that does not fit the first one's buffer: the early count says so while the first emit may
    still be writing the old buffer, which is freed only after a synchronisation; the second emit gives the oracle's soup"""
    from invesalius3_amd.device import DeviceVolume
    img = _image(shape)
    seed = tuple(int(v) for v in np.unravel_index(int(np.argmax(img)), img.shape))
    lo_small, lo_big = int(np.percentile(img, 99)), int(np.percentile(img, 60))
    small, big = (_expected(oracle, img, lo, HI, seed) for lo in (lo_small, lo_big))
    assert len(small[1]) > 0 and len(big[1]) * 36 > int(len(small[1]) * 36 * 1.25) + 4096
    vol = DeviceVolume(img)
    for k, (lo, want) in enumerate(((lo_small, small), (lo_small, small), (lo_big, big))):
        before = vol._tris.nbytes if vol._tris is not None else None
        vol.zero_out_mask()
        vol.threshold(lo, HI)
        vol.region_grow([seed[::-1]], lo, HI, S26, fill=1, select_value=254)
        assert vol.marching_cubes(from_binary=True) == len(want[1])
        if k == 1:
            assert vol._tris.nbytes == before  # steady state
        if k == 2:
            assert before < len(big[1]) * 36 <= vol._tris.nbytes
    vol.sync()
    _cmp(vol._tris.download((len(big[1]), 3, 3), np.float32), big[1])
    _cmp(vol.download_mask(), big[0])
    vol.close()
