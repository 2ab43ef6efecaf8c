"""The use-mode threshold with one plane word per lane (csrc/words_from_records.h: k_threshold16_plane_use and, for a click with
thresholds of its own and no barrier, k_flood_candidates_words): a wave classifies 64 words from their records, packs its mixed
words eight to a load instruction, eight lanes to a word, ORs the lanes' bytes together and hands each word to its owner lane.

Every case builds the records with the build mode of ivx_dev_threshold_i16_plane_ranges, runs use mode into a plane filled with
0x5a and compares it bit for bit with numpy's (img >= lo) & (img <= hi), packed little-endian along x, and with the build-mode
plane; then it runs ivx_dev_flood_candidates_ranges with bar_mode 0 and 1 on the same records against numpy's
in-range & (bar != fill).  The shapes are the smallest at which the kernel takes another path: a wave is 64 words, a workgroup
256, a pass 8 mixed words, and the pass bodies switch at 8, 16, 24, 32 and 48 mixed words in a wave."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LO, HI = 226, 3071
BUILD, USE = 0, 1
FILL = 3
OUT, IN, MIXED = 0, 1, 2
c64 = ctypes.c_int64


def _inr(img, lo, hi):
    a = img.astype(np.int32)
    return (a >= lo) & (a <= hi)


def _plane(inr):
    return np.packbits(np.asarray(inr, bool).reshape(-1, 8), axis=1, bitorder="little").reshape(-1)


def _words(kinds, seed=0):
    """(len(kinds), 64) int16: OUT words below LO or above HI in turn, IN words inside, MIXED words straddling LO with at
    least one voxel on each side"""
    kinds = np.asarray(kinds)
    nw = len(kinds)
    rng = np.random.default_rng(seed + nw)
    base = np.where(kinds == OUT, np.where(np.arange(nw) % 2, 3500, -900), np.where(kinds == IN, 1500, LO)).astype(np.int16)
    w = base[:, None] + rng.integers(-40, 41, (nw, 64)).astype(np.int16)
    for i in np.flatnonzero(kinds == MIXED):
        a, b = rng.choice(64, 2, replace=False)
        w[i, a], w[i, b] = LO - 1, LO
    return w


def _decided(nw):
    """IN and OUT in alternation"""
    return np.arange(nw) % 2


def _check(L, img, lo, hi, kinds=None):
    """build mode, use mode and both candidate passes on `img`; `kinds`: what each word's voxels are with (lo, hi), checked
    first so that a case holds the words its name says"""
    from invesalius3_amd.device import DeviceBuffer
    lib, n, nw = L.lib(), img.size, img.size // 64
    dims = [c64(v) for v in img.shape]
    inr = _inr(img, lo, hi)
    if kinds is not None:
        wi = inr.reshape(-1, 64)
        got = np.where(wi.all(axis=1), IN, np.where(wi.any(axis=1), MIXED, OUT))
        assert np.array_equal(got, kinds)
    want = _plane(inr)
    rng = np.random.default_rng(11)
    bar = np.where(rng.random(img.shape) < 0.2, FILL, rng.integers(0, 3, img.shape)).astype(np.uint8)
    d_img, d_bits, d_rec, d_bar = DeviceBuffer(n * 2), DeviceBuffer(n // 8), DeviceBuffer(nw * 4), DeviceBuffer(n)
    d_img.upload(img)
    d_bar.upload(bar)
    try:
        planes = []
        for mode in (BUILD, USE):
            L.check(lib.ivx_memset(d_bits.ptr, 0x5a, ctypes.c_size_t(n // 8), None))
            L.check(lib.ivx_dev_threshold_i16_plane_ranges(d_img.ptr, *dims, int(lo), int(hi), d_bits.ptr, d_rec.ptr, mode, None),
                    "plane_ranges")
            L.check(lib.ivx_device_synchronize())
            planes.append(d_bits.download((n // 8,), np.uint8))
        bad = np.flatnonzero(planes[USE] != want)
        assert bad.size == 0, "use mode: %d plane bytes differ from numpy, first at byte %d (word %d): got %#x want %#x" % (
            bad.size, bad[0], bad[0] // 8, planes[USE][bad[0]], want[bad[0]])
        assert np.array_equal(planes[BUILD], want)
        assert np.array_equal(planes[USE], planes[BUILD])
        # the candidate pass reads the same records; its double bounds are rounded inwards, so +-0.5 gives [lo, hi]
        plan = L.FloodPlan(*img.shape, img.shape[2] // 64, 0)
        for bar_mode in (0, 1):
            L.check(lib.ivx_memset(d_bits.ptr, 0x5a, ctypes.c_size_t(n // 8), None))
            L.check(lib.ivx_dev_flood_candidates_ranges(ctypes.byref(plan), d_img.ptr, ctypes.c_double(lo - 0.5), ctypes.c_double(hi + 0.5),
                                                        d_bar.ptr if bar_mode else None, bar_mode, ctypes.c_double(FILL), d_rec.ptr,
                                                        d_bits.ptr, None), "candidates_ranges")
            L.check(lib.ivx_device_synchronize())
            cand = d_bits.download((n // 8,), np.uint8)
            assert np.array_equal(cand, _plane(inr & (bar != FILL)) if bar_mode else want), "candidates, bar_mode %d" % bar_mode
    finally:
        for d in (d_img, d_bits, d_rec, d_bar):
            d.close()


# ---- word counts: a partial wave, a full one, a wave boundary, a second workgroup, rows of three words -----------------------
@pytest.mark.parametrize("shape", [(1, 1, 64), (1, 3, 64), (1, 63, 64), (1, 64, 64), (1, 65, 64), (1, 257, 64), (2, 3, 192)])
def test_word_counts(ivxlib, shape):
    nw = int(np.prod(shape)) // 64
    kinds = np.random.default_rng(nw).integers(0, 3, nw)
    kinds[nw - 1] = MIXED
    _check(ivxlib, _words(kinds).reshape(shape), LO, HI, kinds)


# ---- bit assembly: every byte, segment and owner hand-over once ------------------------------------------------------------------
@pytest.mark.parametrize("one", ["in range", "out of range"])
def test_one_voxel_per_word_at_its_own_position(ivxlib, one):
    w = np.full((64, 64), -900 if one == "in range" else 1500, np.int16)
    w[np.arange(64), np.arange(64)] = 1500 if one == "in range" else -900
    _check(ivxlib, w.reshape(1, 64, 64), LO, HI, np.full(64, MIXED))


# ---- packing: how many mixed words a wave holds, and where ---------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first lanes", "last lanes", "scattered"])
@pytest.mark.parametrize("nmix", [0, 1, 7, 8, 9, 16, 17, 24, 25, 32, 33, 40, 48, 49, 64])  # every switch between pass bodies
def test_mixed_words_of_one_wave(ivxlib, nmix, where):
    kinds = _decided(64)
    at = {"first lanes": np.arange(nmix), "last lanes": np.arange(64 - nmix, 64),
          "scattered": np.random.default_rng(100 + nmix).choice(64, nmix, replace=False)}[where]
    kinds[at] = MIXED
    _check(ivxlib, _words(kinds, seed=nmix).reshape(1, 64, 64), LO, HI, kinds)


# ---- the edges of a partial wave and of a workgroup -------------------------------------------------------------------------------
@pytest.mark.parametrize("others", ["decided", "mixed"])
def test_last_valid_lane_and_first_lane_of_the_second_workgroup(ivxlib, others):
    nw = 256 + 64 + 6  # the last wave holds 6 words
    kinds = _decided(nw) if others == "decided" else np.full(nw, MIXED)
    kinds[[nw - 1, 256]] = MIXED
    kinds[[nw - 2, 255, 257]] = (IN, OUT, IN)
    _check(ivxlib, _words(kinds).reshape(1, nw, 64), LO, HI, kinds)


# ---- values ----------------------------------------------------------------------------------------------------------------------------
def _value_image():
    """65 words around lo = 100, hi = 200 with the bounds' neighbours and int16's ends among them"""
    lo, hi = 100, 200
    rng = np.random.default_rng(5)
    w = rng.integers(lo - 60, hi + 60, (65, 64)).astype(np.int16)
    w[0:8] = rng.integers(lo, hi + 1, (8, 64))          # inside
    w[8:16] = rng.integers(hi + 1, hi + 300, (8, 64))   # outside
    w[0, 7], w[1, 63] = lo, hi                          # inside, at the bounds
    w[8, 0], w[9, 5] = hi + 1, 32767                    # outside, touching
    w[10] = rng.integers(-300, lo, 64)
    w[10, 9], w[10, 63] = lo - 1, -32768
    for i, v in enumerate((lo - 1, lo, hi, hi + 1, -32768, 32767)):
        w[20 + i, 8 * i + i] = v                        # one of each in a mixed word, in its own segment
    w[30] = lo                                          # lo == hi == every voxel
    w[31, :2] = (-32768, 32767)
    return w.reshape(1, 65, 64), lo, hi


@pytest.mark.parametrize("bounds", ["lo..hi", "lo==hi", "lo>hi", "beyond int16", "all outside", "only 32767", "only -32768"])
def test_values_at_the_bounds(ivxlib, bounds):
    img, lo, hi = _value_image()
    lo_hi = {"lo..hi": (lo, hi), "lo==hi": (lo, lo), "lo>hi": (hi, lo), "beyond int16": (-40000, 40000), "all outside": (40000, 50000),
             "only 32767": (32767, 40000), "only -32768": (-40000, -32768)}[bounds]
    kinds = None
    if bounds in ("lo>hi", "all outside"):
        kinds = np.full(65, OUT)  # every word decided
    if bounds == "beyond int16":
        kinds = np.full(65, IN)
    _check(ivxlib, img, *lo_hi, kinds)
