"""The mask's bytes written once per step: the plane-only thresholds (csrc/k_threshold.hip), the pass that writes every byte of
the mask from its planes (ivx_dev_mask_from_planes, csrc/k_flood.hip) and the `_mask_pending` note of DeviceVolume that joins
them.  Everything is bit-exact; kernel expectations are numpy's, state expectations are numpy's, the oracle's and those of a
second volume built with IVX_MASK_DEFER=0.

Not tested here: the grid-stride trip of ivx_dev_mask_from_planes (more than 16384 x 1024 chunks = 268 M voxels); bench.py's
`other_configs.grow_mc_1024` runs it and gates on parity."""
import ctypes

import numpy as np
import pytest
from scipy.ndimage import generate_binary_structure

pytestmark = pytest.mark.gpu
S26 = generate_binary_structure(3, 3).astype(np.uint8)
LO, HI = 226, 3071
BUILD, USE = 0, 1
c64 = ctypes.c_int64
# one quad; fewer chunks than a workgroup; odd rows, two words per row; three words per row; more than 16384 x 256 chunks (the
# grid-stride loop's second trip)
T_SHAPES = [(1, 1, 64), (3, 5, 64), (5, 33, 128), (20, 48, 192), (264, 512, 512)]
# one quad; fewer chunks than a workgroup; 1300 chunks = one full 1024-chunk trip of a block and a ragged 276-chunk tail
P_SHAPES = [(1, 1, 64), (3, 5, 64), (5, 13, 320)]


def _inr(img, lo, hi):
    return (img >= lo) & (img <= hi)


def _plane(inr):
    return np.packbits(np.asarray(inr, bool).reshape(-1, 8), axis=1, bitorder="little").reshape(-1)


def _records(img):
    w = img.reshape(-1, 64)
    return w.min(axis=1).view(np.uint16).astype(np.uint32) | (w.max(axis=1).view(np.uint16).astype(np.uint32) << 16)


def _image(shape):
    """words below the range, above it, wholly inside and straddling LO next to each other (one word: straddling), +-40 of noise"""
    nw = int(np.prod(shape)) // 64
    rng = np.random.default_rng(shape[0] * 7 + shape[2])
    kind = rng.integers(0, 4, nw) if nw > 4 else np.arange(3, 3 - nw, -1)
    base = np.array([-900, 3500, 1500, LO], np.int16)[kind]
    noise = rng.integers(-40, 41, (4096, 64)).astype(np.int16)
    return (base[:, None] + noise[np.arange(nw) % 4096]).reshape(shape)


def _mask_want(img, lo, hi):
    return (_inr(img, lo, hi) * np.uint8(255)).astype(np.uint8)


class _Bufs:
    def __init__(self, L, img):
        from invesalius3_amd.device import DeviceBuffer
        self.L, self.lib, self.shape, self.n = L, L.lib(), img.shape, img.size
        self.img, self.mask, self.bits, self.bits2, self.rec, self.rec2 = (
            DeviceBuffer(self.n * 2), DeviceBuffer(self.n), DeviceBuffer(self.n // 8), DeviceBuffer(self.n // 8),
            DeviceBuffer(self.n // 16), DeviceBuffer(self.n // 16))
        self.img.upload(img)
        self.dims = [c64(v) for v in img.shape]

    def plane(self, lo, hi, mode):
        """the plane-only threshold (mode None: the form without records) into a plane filled with 0x5a"""
        L, lib = self.L, self.lib
        L.check(lib.ivx_memset(self.bits.ptr, 0x5a, ctypes.c_size_t(self.n // 8), None))
        if mode is None:
            L.check(lib.ivx_dev_threshold_i16_plane(self.img.ptr, *self.dims, int(lo), int(hi), self.bits.ptr, None), "plane")
        else:
            L.check(lib.ivx_dev_threshold_i16_plane_ranges(self.img.ptr, *self.dims, int(lo), int(hi), self.bits.ptr, self.rec.ptr,
                                                           mode, None), "plane_ranges")
        L.check(lib.ivx_device_synchronize())
        return self.bits.download((self.n // 8,), np.uint8)

    def fused_plane(self, lo, hi, mode):
        """the plane ivx_dev_threshold_i16_bits_ranges writes, with records of its own"""
        L, lib = self.L, self.lib
        L.check(lib.ivx_dev_threshold_i16_bits_ranges(self.img.ptr, *self.dims, int(lo), int(hi), self.mask.ptr, self.bits2.ptr,
                                                      self.rec2.ptr, mode, None), "bits_ranges")
        L.check(lib.ivx_device_synchronize())
        return self.bits2.download((self.n // 8,), np.uint8)

    def close(self):
        for b in (self.img, self.mask, self.bits, self.bits2, self.rec, self.rec2):
            b.close()


# ---- the plane-only thresholds -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", T_SHAPES)
def test_plane_only_threshold_equals_numpy_and_the_fused_kernel(ivxlib, shape):
    img = _image(shape)
    w = img.reshape(-1, 64)
    nw = len(w)
    if nw > 4:  # words of every kind
        full, none = _inr(w, LO, HI).all(axis=1), ~_inr(w, LO, HI).any(axis=1)
        assert full.any() and none.any() and (~full & ~none).any()
    k = nw // 2
    bounds = [(LO + 30, 1520), (1500, 1500), (-32768, 32767), (int(w[k].min()), int(w[k].max()))]
    if nw > 100000:
        bounds = bounds[::3]  # (numpy's side of the large shape takes a second per pair)
    L, lib = ivxlib, ivxlib.lib()
    b = _Bufs(L, img)
    # BUILD: the plane, and the records of ivx_dev_image_ranges_i16
    b.rec.zero()
    assert np.array_equal(b.plane(LO, HI, BUILD), _plane(_inr(img, LO, HI)))
    assert np.array_equal(b.bits.download((b.n // 8,), np.uint8), b.fused_plane(LO, HI, BUILD))
    rec = b.rec.download((nw,), np.uint32)
    L.check(lib.ivx_dev_image_ranges_i16(b.img.ptr, *b.dims, b.rec2.ptr, None), "image_ranges")
    L.check(lib.ivx_device_synchronize())
    assert np.array_equal(rec, b.rec2.download((nw,), np.uint32)) and np.array_equal(rec, _records(img))
    # USE and the form without records
    for lo, hi in bounds:
        want = _plane(_inr(img, lo, hi))
        assert np.array_equal(b.plane(lo, hi, USE), want), (lo, hi)
        assert np.array_equal(b.plane(lo, hi, None), want), (lo, hi)
        assert np.array_equal(b.fused_plane(lo, hi, USE), want), (lo, hi)
    assert np.array_equal(b.rec.download((nw,), np.uint32), rec)  # (use mode leaves the records alone)
    b.close()


def test_plane_use_mode_answers_from_the_records_where_they_decide(ivxlib):
    """the image is changed behind the records: every word the records decide comes out as they say, so no voxel was read there
    (a silent fall-back to the full pass would pass every other test here); the mixed words show the new voxels"""
    img = _image((5, 33, 128))
    b = _Bufs(ivxlib, img)
    b.plane(LO, HI, BUILD)
    w = img.reshape(-1, 64)
    full, none = _inr(w, LO, HI).all(axis=1), ~_inr(w, LO, HI).any(axis=1)
    img2 = np.where(full[:, None], np.int16(-900), np.where(none[:, None], np.int16(1500), w + np.int16(50))).astype(np.int16)
    b.img.upload(img2)
    got = b.plane(LO, HI, USE).reshape(-1, 8)
    want = _plane(_inr(img2, LO, HI)).reshape(-1, 8)
    assert (want[full] == 0).all() and (want[none] == 255).all()
    want[full], want[none] = 255, 0
    assert full.sum() > 3 and none.sum() > 3 and np.array_equal(got, want)
    b.close()


# ---- every byte of the mask from its planes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("reached_case", ["null", "empty", "equal to inside", "subset of inside", "bits outside inside"])
@pytest.mark.parametrize("shape", P_SHAPES)
def test_mask_from_planes_writes_every_byte(ivxlib, shape, reached_case):
    from invesalius3_amd.device import DeviceBuffer
    L, lib = ivxlib, ivxlib.lib()
    n = int(np.prod(shape))
    rng = np.random.default_rng(n + len(reached_case))
    kind = rng.integers(0, 3, n // 16)  # chunks without a bit, full ones and mixed ones
    inside = np.where(kind[:, None] == 0, False, np.where(kind[:, None] == 1, True, rng.random((n // 16, 16)) < 0.5)).reshape(-1)
    reached = {"null": None, "empty": np.zeros(n, bool), "equal to inside": inside, "subset of inside": inside & (rng.random(n) < 0.4),
               "bits outside inside": rng.random(n) < 0.3}[reached_case]
    d_in, d_re, d_mask = DeviceBuffer(n // 8), DeviceBuffer(n // 8), DeviceBuffer(n)
    d_in.upload(_plane(inside))
    if reached is not None:
        d_re.upload(_plane(reached))
    plan = L.FloodPlan(*shape, shape[2] // 64, 0)
    for v_in, v_sel in ((255, 254), (255, 1), (7, 0)):
        L.check(lib.ivx_memset(d_mask.ptr, 0xAA, ctypes.c_size_t(n), None))
        L.check(lib.ivx_dev_mask_from_planes(ctypes.byref(plan), d_in.ptr, d_re.ptr if reached is not None else None, d_mask.ptr,
                                             v_in, v_sel, None), "mask_from_planes")
        L.check(lib.ivx_device_synchronize())
        want = np.where(inside, np.uint8(v_in), np.uint8(0))
        if reached is not None:
            want = np.where(reached, np.uint8(v_sel), want)  # (v_sel wins outside the inside plane too, as in the flood's apply)
        assert np.array_equal(d_mask.download((n,), np.uint8), want.astype(np.uint8)), (v_in, v_sel)
    for d in (d_in, d_re, d_mask):
        d.close()


def test_refusals_launch_nothing(ivxlib):
    from invesalius3_amd.device import DeviceBuffer
    L, lib = ivxlib, ivxlib.lib()
    d, out = DeviceBuffer(1 << 16), DeviceBuffer(1 << 16)
    L.check(lib.ivx_memset(out.ptr, 0xAA, ctypes.c_size_t(1 << 16), None))
    odd = ctypes.c_void_p(out.ptr.value + 8)
    z, y, x = c64(2), c64(4), c64(64)
    plan, ragged = L.FloodPlan(2, 4, 64, 1, 0), L.FloodPlan(2, 4, 48, 1, 0)
    rcs = [lib.ivx_dev_threshold_i16_plane(d.ptr, z, y, c64(48), 0, 1, out.ptr, None),
           lib.ivx_dev_threshold_i16_plane(d.ptr, z, y, x, 0, 1, odd, None),
           lib.ivx_dev_threshold_i16_plane(None, z, y, x, 0, 1, out.ptr, None),
           lib.ivx_dev_threshold_i16_plane(d.ptr, z, y, x, 0, 1, None, None),
           lib.ivx_dev_threshold_i16_plane_ranges(d.ptr, z, y, c64(48), 0, 1, out.ptr, out.ptr, USE, None),
           lib.ivx_dev_threshold_i16_plane_ranges(d.ptr, z, y, x, 0, 1, odd, out.ptr, USE, None),
           lib.ivx_dev_threshold_i16_plane_ranges(d.ptr, z, y, x, 0, 1, out.ptr, None, BUILD, None),
           lib.ivx_dev_threshold_i16_plane_ranges(None, z, y, x, 0, 1, out.ptr, out.ptr, BUILD, None),
           lib.ivx_dev_threshold_i16_plane_ranges(d.ptr, z, y, x, 0, 1, out.ptr, out.ptr, 2, None),
           lib.ivx_dev_mask_from_planes(ctypes.byref(ragged), d.ptr, None, out.ptr, 255, 254, None),
           lib.ivx_dev_mask_from_planes(ctypes.byref(plan), d.ptr, None, odd, 255, 254, None),
           lib.ivx_dev_mask_from_planes(ctypes.byref(plan), None, d.ptr, out.ptr, 255, 254, None),
           lib.ivx_dev_mask_from_planes(ctypes.byref(plan), d.ptr, None, None, 255, 254, None),
           lib.ivx_dev_mask_from_planes(ctypes.byref(plan), d.ptr, None, out.ptr, 256, 254, None)]
    assert rcs == [L.IVX_EINVAL] * len(rcs)
    L.check(lib.ivx_device_synchronize())
    assert (out.download((1 << 16,), np.uint8) == 0xAA).all()
    d.close()
    out.close()


# ---- the note in DeviceVolume ---------------------------------------------------------------------------------------------
STATE_SHAPES = [(5, 33, 128), (20, 48, 128)]


def _volumes(monkeypatch, img, slab=False):
    """(a volume with deferral, one built under IVX_MASK_DEFER=0)"""
    from invesalius3_amd.device import DeviceVolume
    if slab:
        from invesalius3_amd.parallel import SlabVolume
        make = lambda: SlabVolume(img, 0, 1)  # noqa: E731
    else:
        make = lambda: DeviceVolume(img)  # noqa: E731
    monkeypatch.delenv("IVX_MASK_DEFER", raising=False)
    vol = make()
    monkeypatch.setenv("IVX_MASK_DEFER", "0")
    off = make()
    monkeypatch.delenv("IVX_MASK_DEFER")
    assert vol._mask_defer and not off._mask_defer
    return vol, off


def _img(shape):
    from conftest import synth_volume
    return synth_volume(shape, seed=77)


def _outside_write(L, vol, sel, value):
    """an outside kernel on mask.ptr: mask[sel == 1] = value"""
    from invesalius3_amd.device import DeviceBuffer
    d = DeviceBuffer(vol.n)
    d.upload(sel)
    L.check(L.lib().ivx_dev_flood_apply_where(vol.mask.ptr, d.ptr, c64(vol.n), 1, int(value), vol.stream))
    vol.sync()
    d.close()


@pytest.mark.parametrize("reader", ["download_mask", "mask.download", "mask.ptr + kernel", "mask.upload", "preserve", "mc from voxels",
                                    "maskren cells", "watershed", "mask_bytes"])
@pytest.mark.parametrize("shape", STATE_SHAPES)
def test_every_reader_sees_the_thresholds_bytes(ivxlib, monkeypatch, shape, reader):
    L, lib = ivxlib, ivxlib.lib()
    img = _img(shape)
    lo, hi = -700, 3071
    want = _mask_want(img, lo, hi)
    assert 0 < int((want == 255).sum()) < img.size
    vol, off = _volumes(monkeypatch, img)
    rng = np.random.default_rng(3)
    sel, other = (rng.random(shape) < 0.1).astype(np.uint8), rng.integers(0, 256, shape).astype(np.uint8)
    got = []
    for v in (vol, off):
        v.threshold(lo, hi)
        assert v._mask_pending == (v is vol)
        if reader == "download_mask":
            got.append(v.download_mask())
            assert np.array_equal(got[-1], want)
        elif reader == "mask.download":
            if v is off:
                v.sync()  # (nothing pending: a download does not wait for the volume's stream by itself)
            got.append(v.mask.download(shape, np.uint8))
            assert np.array_equal(got[-1], want)
        elif reader == "mask.ptr + kernel":
            _outside_write(L, v, sel, 7)
            got.append(v.download_mask())
            assert np.array_equal(got[-1], np.where(sel == 1, np.uint8(7), want))
        elif reader == "mask.upload":
            v.mask.upload(other)
            got.append(v.download_mask())
            assert np.array_equal(got[-1], other)
        elif reader == "preserve":
            v.threshold(lo + 300, hi, preserve=True)  # nothing to keep in a 0 / 255 mask: the new threshold, byte for byte
            assert not v._mask_pending
            got.append(v.download_mask())
            assert np.array_equal(got[-1], _mask_want(img, lo + 300, hi))
        elif reader == "mc from voxels":
            monkeypatch.setenv("IVX_MC_LEVELS", "0")
            got.append(v.marching_cubes(from_binary=True, download=True).copy())
            monkeypatch.delenv("IVX_MC_LEVELS")
            assert len(got[-1]) > 0 and np.array_equal(v.download_mask(), want)
        elif reader == "maskren cells":
            from invesalius3_amd import volume as V
            ncell = int(np.prod([-(-(s + 1) // V.CELL) for s in shape]))
            cells = v._maskren_cells(1)
            v.sync()
            got.append(cells.download((ncell,), np.uint16))
        elif reader == "watershed":
            mk = np.zeros(shape, np.int8)
            z, y, x = (int(t) for t in np.unravel_index(np.argmax(img), shape))
            mk[z, y, x], mk[0, 0, 0] = 1, 2
            v.watershed(mk, generate_binary_structure(3, 1))
            got.append(v.download_mask())
            assert np.array_equal(got[-1] == 255, want == 255) and np.isin(got[-1][want == 0], (0, 2, 253)).all()
            assert (got[-1] != want).any()
        else:
            p = v.mask_bytes()
            assert p.value == v.mask.raw.value and v._mask_levels == (255, None)  # the bytes are there and the notes are kept
            v.sync()
            got.append(v.mask.download(shape, np.uint8))
            assert np.array_equal(got[-1], want)
        assert not v._mask_pending
    assert np.array_equal(got[0], got[1])
    vol.close()
    off.close()


def test_a_second_threshold_replaces_the_note_without_writing(ivxlib, monkeypatch):
    img = _img(STATE_SHAPES[1])
    vol, off = _volumes(monkeypatch, img)
    vol.sync()
    vol.timer.collect()
    vol.threshold(-700, 3071)
    assert vol._mask_pending
    vol.threshold(-300, 2000)
    assert vol._mask_pending
    assert np.array_equal(vol.download_mask(), _mask_want(img, -300, 2000))
    assert not vol._mask_pending and len(vol.timer.collect().get("mask_bytes", [])) == 1
    off.threshold(-300, 2000)
    assert np.array_equal(off.download_mask(), _mask_want(img, -300, 2000)) and "mask_bytes" not in off.timer.collect()
    vol.close()
    off.close()


@pytest.mark.parametrize("slab", [False, True], ids=["volume", "slab"])
@pytest.mark.parametrize("case", ["shared 254", "own thresholds 254", "shared 1", "shared None"])
@pytest.mark.parametrize("shape", STATE_SHAPES)
def test_region_grow_after_a_deferred_threshold_equals_the_oracle(ivxlib, oracle, monkeypatch, shape, case, slab):
    img = _img(shape)
    z, y, x = (int(v) for v in np.unravel_index(np.argmax(img), shape))
    t0, t1 = int(img[z, y, x]) - 900, 3071
    m0 = t0 if case.startswith("shared") else t0 + 200  # the mask's own lower threshold
    sel = {"254": 254, "1": 1, "None": None}[case.split()[-1]]
    ref = np.zeros(shape, np.uint8)
    oracle.floodfill_threshold(img, [(x, y, z)], t0, t1, 1, S26, ref)
    assert 0 < int(ref.sum()) < img.size
    want = _mask_want(img, m0, t1)
    if sel is not None:
        want[ref == 1] = sel
    vol, off = _volumes(monkeypatch, img, slab)
    for v in (vol, off):
        v.zero_out_mask()
        v.threshold(m0, t1)
        assert v._mask_pending == (v is vol)
        v.region_grow([(x, y, z)], t0, t1, S26, fill=1, select_value=sel)
        assert not v._mask_pending
        assert v._mask_levels == {254: (255, 254), 1: None, None: (255, None)}[sel]
        assert np.array_equal(v.download_mask(), want)
        assert np.array_equal(v.download_out_mask(), ref)
        if sel == 1:  # _mbits was combined: the inside plane is the mask's again
            assert np.array_equal(v._mbits.download((v.n // 8,), np.uint8), _plane(want >= 127))
    # a second flood right after the first: the note of the first leant on the reached plane that is cleared now
    if sel == 254:
        for v in (vol, off):
            v.zero_out_mask()
            v.region_grow([(x, y, z)], t0 + 400, t1, S26, fill=1, select_value=253)
            assert not v._mask_pending
        ref2 = np.zeros(shape, np.uint8)
        oracle.floodfill_threshold(img, [(x, y, z)], t0 + 400, t1, 1, S26, ref2)
        want[ref2 == 1] = 253
        assert np.array_equal(vol.download_mask(), want) and np.array_equal(off.download_mask(), want)
    vol.close()
    off.close()


@pytest.mark.parametrize("slab", [False, True], ids=["volume", "slab"])
@pytest.mark.parametrize("shape", STATE_SHAPES)
def test_marching_cubes_without_a_flood_leaves_the_mask_written(ivxlib, monkeypatch, shape, slab):
    img = _img(shape)
    vol, off = _volumes(monkeypatch, img, slab)
    n = []
    for v in (vol, off):
        v.threshold(-700, 3071)
        n.append(v.marching_cubes(from_binary=True))
        assert not v._mask_pending
        assert np.array_equal(v.download_mask(), _mask_want(img, -700, 3071))
    assert n[0] == n[1] > 0
    vol.close()
    off.close()


def test_ragged_rows_and_preserve_never_set_the_note(ivxlib, monkeypatch):
    from invesalius3_amd.device import DeviceVolume
    monkeypatch.delenv("IVX_MASK_DEFER", raising=False)
    ragged = np.ascontiguousarray(_img((5, 33, 128))[:, :, :48])
    vol = DeviceVolume(ragged)
    vol.threshold(-700, 3071)
    assert not vol._mask_pending and np.array_equal(vol.download_mask(), _mask_want(ragged, -700, 3071))
    vol.close()
    img = _img((5, 33, 128))
    vol = DeviceVolume(img)
    vol.threshold(-700, 3071, preserve=True)
    assert not vol._mask_pending and np.array_equal(vol.download_mask(), _mask_want(img, -700, 3071))
    vol.close()


def test_deferral_follows_whether_a_flood_consumed_the_last_note(ivxlib, oracle, monkeypatch):
    """a threshold whose bytes needed a pass of their own is followed by fused ones (threshold + marching cubes steps stay what
    they were), until a region growing meets a threshold's mask again"""
    img = _img(STATE_SHAPES[1])
    z, y, x = (int(v) for v in np.unravel_index(np.argmax(img), img.shape))
    t0, t1 = int(img[z, y, x]) - 900, 3071
    vol, off = _volumes(monkeypatch, img)
    off.close()
    vol.threshold(t0, t1)
    assert vol._mask_pending
    vol.marching_cubes(from_binary=True)  # writes the bytes itself
    vol.sync()
    vol.timer.collect()
    vol.threshold(t0 + 100, t1)
    assert not vol._mask_pending  # the fused kernel
    vol.marching_cubes(from_binary=True)
    assert np.array_equal(vol.download_mask(), _mask_want(img, t0 + 100, t1)) and "mask_bytes" not in vol.timer.collect()
    vol.zero_out_mask()
    vol.threshold(t0, t1)
    assert not vol._mask_pending
    vol.region_grow([(x, y, z)], t0, t1, S26, fill=1, select_value=254)  # today's apply, on a mask that a deferral would have served
    vol.zero_out_mask()
    vol.threshold(t0, t1)
    assert vol._mask_pending
    vol.region_grow([(x, y, z)], t0, t1, S26, fill=1, select_value=254)
    ref = np.zeros(img.shape, np.uint8)
    oracle.floodfill_threshold(img, [(x, y, z)], t0, t1, 1, S26, ref)
    want = _mask_want(img, t0, t1)
    want[ref == 1] = 254
    assert not vol._mask_pending and np.array_equal(vol.download_mask(), want)
    vol.close()
