"""The per-word (min, max) records of the resident image (csrc/k_threshold.hip): one int16 pair per 64-voxel x-word, written by
the first threshold after the image's bytes changed (build mode) and read by every later one (use mode), which loads voxels of
mixed words only.  Also the candidate pass of a click with thresholds of its own (k_flood_candidates16_ranges) and the
bookkeeping in DeviceVolume that decides when the records may be trusted.  Every expected value is numpy's."""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
from scipy.ndimage import generate_binary_structure

pytestmark = pytest.mark.gpu
S26 = generate_binary_structure(3, 3).astype(np.uint8)
# one word per row and fewer chunks than one workgroup; odd row counts; three words per row; more than 16384 x 256 chunks
# (the grid-stride loop's second trip)
SHAPES = [(3, 5, 64), (5, 33, 128), (20, 48, 192), (264, 512, 512)]
LO, HI = 226, 3071
BUILD, USE = 0, 1
c64 = ctypes.c_int64


def _inr(img, lo, hi):
    a = img if -32768 <= lo <= 32767 and -32768 <= hi <= 32767 else img.astype(np.int32)
    return (a >= lo) & (a <= hi)


def _want(img, lo, hi):
    """(mask bytes, plane as bytes) of the threshold"""
    inr = _inr(img, lo, hi)
    return (inr * np.uint8(255)).astype(np.uint8), np.packbits(inr.reshape(-1, 8), axis=1, bitorder="little").reshape(-1)


def _records(img):
    w = img.reshape(-1, 64)
    return w.min(axis=1).view(np.uint16).astype(np.uint32) | (w.max(axis=1).view(np.uint16).astype(np.uint32) << 16)


def _rec(mn, mx):
    return np.uint32((int(mn) & 0xffff) | ((int(mx) & 0xffff) << 16))


def _image(shape):
    """words of every kind next to each other: a quarter each below the range, above it, wholly inside and straddling `LO`,
    each with +-40 of noise; the int16 ends as the minimum of one word and the maximum of another, also in the last word"""
    nw = int(np.prod(shape)) // 64
    rng = np.random.default_rng(shape[0] * 7 + shape[2])
    kind = rng.integers(0, 4, nw)
    base = np.array([-900, 3500, 1500, LO], np.int16)[kind]
    noise = rng.integers(-40, 41, (4096, 64)).astype(np.int16)
    img = base[:, None] + noise[np.arange(nw) % 4096]
    img[0, 5], img[1 % nw, 63], img[nw - 1, 0], img[nw - 1, 63] = -32768, 32767, 32767, -32768
    return img.reshape(shape)


class _Bufs:
    """the image on the device with a mask, a plane and a record buffer"""

    def __init__(self, L, img):
        from invesalius3_amd.device import DeviceBuffer
        self.L, self.lib, self.shape, self.n = L, L.lib(), img.shape, img.size
        nb = ctypes.c_size_t(0)
        L.check(self.lib.ivx_image_ranges_bytes(*(c64(v) for v in img.shape), ctypes.byref(nb)), "image_ranges_bytes")
        assert nb.value == self.n // 64 * 4
        self.img, self.mask, self.bits, self.rec = (DeviceBuffer(self.n * 2), DeviceBuffer(self.n), DeviceBuffer(self.n // 8),
                                                   DeviceBuffer(nb.value))
        self.img.upload(img)

    def dims(self):
        return [c64(v) for v in self.shape]

    def threshold(self, lo, hi, mode):
        """mode None: ivx_dev_threshold_i16_bits.  -> (mask, plane bytes); the outputs are filled with 0x5a first"""
        L, lib = self.L, self.lib
        L.check(lib.ivx_memset(self.mask.ptr, 0x5a, ctypes.c_size_t(self.n), None))
        L.check(lib.ivx_memset(self.bits.ptr, 0x5a, ctypes.c_size_t(self.n // 8), None))
        if mode is None:
            L.check(lib.ivx_dev_threshold_i16_bits(self.img.ptr, *self.dims(), int(lo), int(hi), self.mask.ptr, self.bits.ptr, None),
                    "threshold_bits")
        else:
            L.check(lib.ivx_dev_threshold_i16_bits_ranges(self.img.ptr, *self.dims(), int(lo), int(hi), self.mask.ptr, self.bits.ptr,
                                                          self.rec.ptr, mode, None), "threshold_bits_ranges")
        L.check(lib.ivx_device_synchronize())
        return self.mask.download(self.shape, np.uint8), self.bits.download((self.n // 8,), np.uint8)

    def records(self):
        return self.rec.download((self.n // 64,), np.uint32)

    def close(self):
        for b in (self.img, self.mask, self.bits, self.rec):
            b.close()


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- the records and the two modes, every shape ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_records_and_both_modes_equal_numpy(ivxlib, shape):
    img = _image(shape)
    want_rec = _records(img)
    assert (want_rec & 0xffff == 0x8000).any() and (want_rec >> 16 == 0x7fff).any()  # the int16 ends as a minimum and as a maximum
    b = _Bufs(ivxlib, img)
    L, lib = ivxlib, ivxlib.lib()
    # stand-alone build
    b.rec.zero()
    L.check(lib.ivx_dev_image_ranges_i16(b.img.ptr, *b.dims(), b.rec.ptr, None), "image_ranges")
    L.check(lib.ivx_device_synchronize())
    assert np.array_equal(b.records(), want_rec)
    # by-product of a build-mode threshold: same records, and the threshold is today's
    b.rec.zero()
    want = _want(img, LO, HI)
    assert _same(b.threshold(LO, HI, BUILD), want)
    assert np.array_equal(b.records(), want_rec)
    # use mode with other thresholds
    lo2, hi2 = LO + 30, 1520
    want2 = _want(img, lo2, hi2)
    assert _same(b.threshold(lo2, hi2, USE), want2)
    assert _same(b.threshold(lo2, hi2, None), want2)
    assert np.array_equal(b.records(), want_rec)  # (use mode leaves them alone)
    b.close()


# ---- every word kind at its edge --------------------------------------------------------------------------------------------
def _edge_image():
    """(4, 6, 128) = 48 words made by hand around lo = 100, hi = 200; -> (image, {name: word index})"""
    lo, hi = 100, 200
    w = np.full((48, 64), 150, np.int16)
    w[:, ::3] = 120
    w[:, 1::5] = 180
    names = {}

    def put(name, i):
        names[name] = i
        return w[i]

    put("min==lo", 0)[7] = lo                      # inside
    put("min==lo-1", 1)[40] = lo - 1               # mixed: exactly one voxel out
    put("max==hi", 2)[63] = hi                     # inside
    put("max==hi+1", 3)[0] = hi + 1                # mixed: exactly one voxel out
    put("max==lo-1", 4)[:] = lo - 1                # wholly outside, touching from below
    w[4, 3] = -500
    put("min==hi+1", 5)[:] = hi + 1                # wholly outside, touching from above
    w[5, 60] = 900
    for k, v in enumerate((0, 15, 16, 63)):        # a mixed word whose only in-range voxel sits at a lane / half boundary
        r = put("only%d" % v, 6 + k)
        r[:] = -20
        r[v] = 150
    put("const==lo", 10)[:] = lo                   # lo == hi == every voxel
    put("ends", 11)[:2] = (-32768, 32767)          # mixed with the int16 ends
    put("low-end", 12)[:] = -32768
    put("high-end", 13)[:] = 32767
    rng = np.random.default_rng(5)
    w[14:] = rng.integers(lo - 60, hi + 60, (34, 64))
    return w.reshape(4, 6, 128), names, lo, hi


@pytest.mark.parametrize("bounds", ["lo..hi", "lo>hi", "lo==hi", "below int16", "above int16", "both beyond", "all out low", "all out high",
                                    "only the ends"])
def test_every_word_kind_at_its_edge(ivxlib, bounds):
    img, names, lo, hi = _edge_image()
    lo_hi = {"lo..hi": (lo, hi), "lo>hi": (hi, lo), "lo==hi": (lo, lo), "below int16": (-40000, hi), "above int16": (lo, 40000),
             "both beyond": (-70000, 70000), "all out low": (-50000, -40000), "all out high": (40000, 50000),
             "only the ends": (32767, 32767)}[bounds]
    w = img.reshape(-1, 64)
    if bounds == "lo..hi":  # the kinds are what their names say
        mn, mx = w.min(axis=1), w.max(axis=1)
        inside, outside = (mn >= lo) & (mx <= hi), (mx < lo) | (mn > hi)
        assert all(inside[names[k]] for k in ("min==lo", "max==hi", "const==lo"))
        assert all(outside[names[k]] for k in ("max==lo-1", "min==hi+1", "low-end", "high-end"))
        assert mx[names["max==lo-1"]] == lo - 1 and mn[names["min==hi+1"]] == hi + 1
        for k in ("min==lo-1", "max==hi+1"):
            assert not inside[names[k]] and not outside[names[k]] and _inr(w[names[k]], lo, hi).sum() == 63
        for v in (0, 15, 16, 63):
            assert np.flatnonzero(_inr(w[names["only%d" % v]], lo, hi)).tolist() == [v]
    b = _Bufs(ivxlib, img)
    want = _want(img, *lo_hi)
    assert _same(b.threshold(*lo_hi, BUILD), want)
    assert np.array_equal(b.records(), _records(img))
    use = b.threshold(*lo_hi, USE)
    assert _same(use, want)
    assert _same(use, b.threshold(*lo_hi, None))  # byte for byte ivx_dev_threshold_i16_bits
    b.close()


# ---- use mode trusts the records --------------------------------------------------------------------------------------------
def test_use_mode_does_not_read_what_the_records_decide(ivxlib):
    """records that lie: "outside" for a word full of in-range voxels, "inside" for a word without one.  Zeros and 255s come
    out there, so the image was not read: a silent fall-back to the full pass would pass every other test here."""
    img = _image((5, 33, 128))
    w = img.reshape(-1, 64)
    full = int(np.flatnonzero(_inr(w, LO, HI).all(axis=1))[3])
    empty = int(np.flatnonzero(~_inr(w, LO, HI).any(axis=1))[3])
    b = _Bufs(ivxlib, img)
    rec = _records(img)
    rec[full], rec[empty] = _rec(HI + 1, HI + 9), _rec(LO, HI)
    b.rec.upload(rec)
    mask, bits = b.threshold(LO, HI, USE)
    want_mask, want_bits = _want(img, LO, HI)
    wm, wb = want_mask.reshape(-1, 64).copy(), want_bits.reshape(-1, 8).copy()
    assert (wm[full] == 255).all() and (wm[empty] == 0).all()
    wm[full], wb[full], wm[empty], wb[empty] = 0, 0, 255, 255
    assert np.array_equal(mask.reshape(-1, 64), wm) and np.array_equal(bits.reshape(-1, 8), wb)
    b.close()


def test_modes_and_shapes_that_are_refused(ivxlib):
    from invesalius3_amd.device import DeviceBuffer
    L, lib = ivxlib, ivxlib.lib()
    d = DeviceBuffer(1 << 16)
    nb = ctypes.c_size_t(0)
    with pytest.raises(TypeError, match="dx % 64"):
        L.check(lib.ivx_image_ranges_bytes(c64(2), c64(4), c64(50), ctypes.byref(nb)), "image_ranges_bytes")
    with pytest.raises(TypeError, match="dx % 64"):
        L.check(lib.ivx_dev_image_ranges_i16(d.ptr, c64(2), c64(4), c64(48), d.ptr, None), "image_ranges")
    with pytest.raises(TypeError, match="dx % 64"):
        L.check(lib.ivx_dev_threshold_i16_bits_ranges(d.ptr, c64(2), c64(4), c64(48), 0, 1, d.ptr, d.ptr, d.ptr, USE, None), "t")
    with pytest.raises(TypeError, match="mode"):
        L.check(lib.ivx_dev_threshold_i16_bits_ranges(d.ptr, c64(2), c64(4), c64(64), 0, 1, d.ptr, d.ptr, d.ptr, 2, None), "t")
    d.close()


# ---- DeviceVolume: when the records may be trusted ---------------------------------------------------------------------------
def _lie(vol, word):
    """make the record of `word` claim "below every threshold": a use-mode threshold then writes zeros there"""
    rec = vol._ranges.download((vol.n // 64,), np.uint32)
    rec[word] = _rec(-32768, -32768)
    vol._ranges.upload(rec)


def _mask_want(img, lo, hi):
    return (_inr(img, lo, hi) * np.uint8(255)).astype(np.uint8)


def test_thresholds_change_on_an_unchanged_image_use_path(ivxlib):
    from invesalius3_amd.device import DeviceVolume
    shape = (20, 48, 192)
    img = _image(shape)
    vol = DeviceVolume(img)
    assert not vol._ranges_valid
    vol.threshold(LO, HI)
    assert vol._ranges_valid and np.array_equal(vol._ranges.download((vol.n // 64,), np.uint32), _records(img))
    assert np.array_equal(vol.download_mask(), _mask_want(img, LO, HI))
    for lo, hi in ((LO + 25, HI), (LO - 30, 1500), (1500, LO), (-40000, 40000)):
        vol.threshold(lo, hi)
        assert np.array_equal(vol.download_mask(), _mask_want(img, lo, hi))
        assert np.array_equal(vol._mbits.download((vol.n // 8,), np.uint8), _want(img, lo, hi)[1])
    # ... and those calls went through the records: a lie shows
    word = int(np.flatnonzero(_inr(img.reshape(-1, 64), LO, HI).all(axis=1))[0])
    _lie(vol, word)
    vol.threshold(LO, HI)
    want = _mask_want(img, LO, HI).reshape(-1, 64).copy()
    want[word] = 0
    assert np.array_equal(vol.download_mask().reshape(-1, 64), want)
    vol.close()


@pytest.mark.parametrize("how", ["upload", "filter_image", "write through image.ptr"])
def test_records_die_with_the_image(ivxlib, how):
    """threshold, change the image's bytes, threshold again: the second one is right.  The stale records are made to lie
    about a word first, so a threshold that still read them would show it."""
    from invesalius3_amd.device import DeviceVolume
    shape = (5, 33, 128)
    img = _image(shape)
    vol = DeviceVolume(img)
    vol.threshold(LO, HI)
    assert vol._ranges_valid
    img2 = np.ascontiguousarray(img[::-1, ::-1, :]) + np.int16(3)
    if how == "upload":
        vol.image.upload(img2)
    elif how == "filter_image":
        from invesalius3_amd import filters as F
        vol.filter_image(F.MEDIAN, 3)
        vol.sync()
        img2 = vol.image.download(shape, np.int16)
        assert not np.array_equal(img2, img)
    else:
        ivxlib.check(ivxlib.lib().ivx_memcpy_h2d(vol.image.ptr, ivxlib.ptr(img2), ctypes.c_size_t(img2.nbytes)))
    assert not vol._ranges_valid
    word = int(np.argmax(_inr(img2.reshape(-1, 64), LO, HI).sum(axis=1)))  # the word with the most in-range voxels
    assert _inr(img2.reshape(-1, 64)[word], LO, HI).any()
    _lie(vol, word)
    vol.threshold(LO, HI)
    assert vol._ranges_valid
    assert np.array_equal(vol.download_mask(), _mask_want(img2, LO, HI))
    assert np.array_equal(vol._ranges.download((vol.n // 64,), np.uint32), _records(img2))
    vol.threshold(LO + 40, HI)  # use mode on the new records
    assert np.array_equal(vol.download_mask(), _mask_want(img2, LO + 40, HI))
    vol.close()


def test_preserve_and_ragged_rows_take_todays_kernels(ivxlib):
    from invesalius3_amd.device import DeviceVolume
    img = _image((5, 33, 128))
    vol = DeviceVolume(img)
    vol.threshold(LO, HI)
    m = vol.download_mask()
    m[1, 2, 3:9], m[2, 4, 60:70] = (1, 2, 253, 254, 7, 255), 254
    vol.mask.upload(m)
    vol.threshold(LO + 40, HI, preserve=True)
    want = _mask_want(img, LO + 40, HI)
    keep = np.isin(m, (1, 2, 253, 254))
    want[keep] = m[keep]
    assert np.array_equal(vol.download_mask(), want)
    vol.close()
    ragged = np.ascontiguousarray(_image((5, 33, 128))[:, :, :100])
    vol = DeviceVolume(ragged)
    vol.threshold(LO, HI)
    vol.threshold(LO + 40, HI)
    assert vol._ranges is None and not vol._ranges_valid
    assert np.array_equal(vol.download_mask(), _mask_want(ragged, LO + 40, HI))
    vol.close()


# ---- the candidate pass --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bar_mode", [0, 1])
@pytest.mark.parametrize("shape", SHAPES[:3])
def test_candidates_from_records_equal_the_plain_pass(ivxlib, shape, bar_mode):
    from invesalius3_amd.device import DeviceBuffer
    L, lib = ivxlib, ivxlib.lib()
    img = _image(shape)
    n = img.size
    rng = np.random.default_rng(11)
    fill = 3
    bar = np.where(rng.random(shape) < 0.2, fill, rng.integers(0, 3, shape)).astype(np.uint8)
    inside = _inr(img.reshape(-1, 64), LO, HI).all(axis=1)
    assert (bar.reshape(-1, 64)[inside] == fill).any()  # barred voxels inside a wholly-inside word
    ok = _inr(img, LO, HI) & ((bar != fill) if bar_mode else True)
    want = np.packbits(ok.reshape(-1, 8), axis=1, bitorder="little").reshape(-1)
    b = _Bufs(L, img)
    b.rec.upload(_records(img))
    d_bar, d_cand = DeviceBuffer(n), DeviceBuffer(n // 8)
    d_bar.upload(bar)
    plan = L.FloodPlan(*shape, shape[2] // 64, 0)
    t0, t1 = ctypes.c_double(LO - 0.5), ctypes.c_double(HI + 0.5)  # (the bounds are rounded inwards for integer data)
    got = []
    for ranges in (True, False):
        L.check(lib.ivx_memset(d_cand.ptr, 0x5a, ctypes.c_size_t(n // 8), None))
        if ranges:
            L.check(lib.ivx_dev_flood_candidates_ranges(ctypes.byref(plan), b.img.ptr, t0, t1, d_bar.ptr if bar_mode else None, bar_mode,
                                                        ctypes.c_double(fill), b.rec.ptr, d_cand.ptr, None), "candidates_ranges")
        else:
            L.check(lib.ivx_dev_flood_candidates(ctypes.byref(plan), L.I16, b.img.ptr, t0, t1, d_bar.ptr if bar_mode else None, bar_mode,
                                                 ctypes.c_double(fill), d_cand.ptr, None), "candidates")
        L.check(lib.ivx_device_synchronize())
        got.append(d_cand.download((n // 8,), np.uint8))
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    for d in (d_bar, d_cand):
        d.close()
    b.close()


def test_region_grow_with_other_thresholds_equals_the_oracle(ivxlib, oracle):
    """the click's thresholds are not the mask's: the candidate plane comes from the records (out_mask known to be zero: no
    barrier is read), then once more into the out_mask the first click left behind (the barrier is read)"""
    from conftest import synth_volume
    from invesalius3_amd.device import DeviceVolume
    shape = (20, 48, 128)
    img = synth_volume(shape, seed=77)
    z, y, x = (int(v) for v in np.unravel_index(np.argmax(img), shape))
    t0, t1 = int(img[z, y, x]) - 900, 3071
    vol = DeviceVolume(img)
    vol.zero_out_mask()
    vol.threshold(t0 + 200, t1)
    assert vol._ranges_valid and vol._out_logically_zero()
    vol.region_grow([(x, y, z)], t0, t1, S26, fill=1, select_value=254)
    ref = np.zeros(shape, np.uint8)
    oracle.floodfill_threshold(img, [(x, y, z)], t0, t1, 1, S26, ref)
    assert 0 < int(ref.sum()) < img.size
    want = _mask_want(img, t0 + 200, t1)
    want[ref == 1] = 254
    assert np.array_equal(vol.download_out_mask(), ref)
    assert np.array_equal(vol.download_mask(), want)
    # a second click into the same out_mask, wider: the first region bars
    assert not vol._out_logically_zero()
    vol.region_grow([(x, y, z)], t0 - 300, t1, S26, fill=1, select_value=254)
    oracle.floodfill_threshold(img, [(x, y, z)], t0 - 300, t1, 1, S26, ref)
    assert np.array_equal(vol.download_out_mask(), ref)
    vol.close()


# ---- the A/B switch ---------------------------------------------------------------------------------------------------------------
def test_switch_off_gives_the_same_mask(ivxlib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, zlib, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from conftest import synth_volume\n"
        "from invesalius3_amd.device import DeviceVolume\n"
        "vol = DeviceVolume(synth_volume((20, 48, 128), seed=5))\n"
        "crc = []\n"
        "for lo in (-700, -400, -400):\n"
        "    vol.threshold(lo, 3071)\n"
        "    crc.append(zlib.crc32(vol.download_mask().tobytes()))\n"
        "print('crc', vol._use_ranges, vol._ranges_valid, *crc)\n") % (root, os.path.join(root, "tests"))
    out = {}
    for flag in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, IVX_RANGES=flag), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out[flag] = [ln for ln in r.stdout.splitlines() if ln.startswith("crc")][0].split()
    assert out["1"][1:3] == ["True", "True"] and out["0"][1:3] == ["False", "False"]
    assert out["1"][3:] == out["0"][3:]
    from conftest import synth_volume
    img = synth_volume((20, 48, 128), seed=5)
    assert [int(v) for v in out["1"][3:]] == [zlib.crc32(_mask_want(img, lo, 3071).tobytes()) for lo in (-700, -400, -400)]
