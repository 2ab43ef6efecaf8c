"""The ordered ray projections (csrc/k_rays.hip) where test_gpu_rays.py does not reach: ray lengths on both sides of the 16-sample
blocks of k_rays_strided, rows on both sides of the LDS chunks of k_rays_rows at aligned and unaligned pointers, waves with dead
lanes, rays built to end at a given sample with a whole wave or a single lane left running, MIDA's min / max pre-pass at its
vector body, scalar tail and block cap, and ivx_dev_fcm_maxip in every FAST variant, on every route, with ragged and 32-fold
segment splits and with pixels only the exact pass k_fcm_fix can settle.  Cases come from _ray_cases.py; test_ray_cases_host.py
proves without a device that each case is where its name says and that the forced-open pictures change when the exact pass is
wrong.  The reference is the C oracle on the same array and every comparison is np.array_equal: the outputs are bit-exact by
design, so there is no tolerance anywhere in this file."""
import ctypes

import numpy as np
import pytest

import _ray_cases as C

pytestmark = pytest.mark.gpu

cdbl, cflt = ctypes.c_double, ctypes.c_float
SENTINEL, GUARD = 0x5A, 64


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d pixels differ from the oracle, first at %s: got %r, oracle %r"
                             % (what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


class Dev:
    """a host array in device memory, `offset` elements past a 256-byte aligned address"""

    def __init__(self, a, offset=0):
        from invesalius3_amd.device import DeviceBuffer
        a = np.ascontiguousarray(a)
        lead = offset * a.itemsize
        raw = np.full(lead + a.nbytes + GUARD, SENTINEL, np.uint8)
        raw[lead:lead + a.nbytes] = a.reshape(-1).view(np.uint8)
        self.buf = DeviceBuffer(raw.size)
        self.buf.upload(raw)
        self.ptr = self.buf.at(lead)
        assert self.buf.ptr.value % 256 == 0 and (self.ptr.value % 16 == 0) == (lead % 16 == 0)

    def close(self):
        self.buf.close()


class Out:
    """an output image of exactly `count` items between sentinel bytes"""

    def __init__(self, count, dtype):
        from invesalius3_amd.device import DeviceBuffer
        self.dtype, self.n = np.dtype(dtype), int(count) * np.dtype(dtype).itemsize
        self.buf = DeviceBuffer(self.n + GUARD)
        self.buf.upload(np.full(self.n + GUARD, SENTINEL, np.uint8))
        self.ptr = self.buf.ptr

    def read(self, shape):
        raw = self.buf.download((self.n + GUARD,), np.uint8)
        assert (raw[self.n:] == SENTINEL).all(), "bytes behind the output image were written"
        self.buf.close()
        return raw[:self.n].copy().view(self.dtype).reshape(shape)


def _oshape(vol, axis):
    return tuple(d for i, d in enumerate(vol.shape) if i != axis)


def _c64(v):
    return ctypes.c_int64(int(v))


def _dims(vol):
    return tuple(_c64(d) for d in vol.shape)


def _status():
    from invesalius3_amd.device import DeviceBuffer
    st = DeviceBuffer(64)
    st.zero()
    return st


def _status_is_zero(L, st):
    L.synchronize()
    word = int(st.download((1,), np.int32)[0])
    st.close()
    assert word == 0, "the status word is %d" % word


def dev_lmip(L, vol, axis, tmin, tmax, offset=0):
    d, out = Dev(vol, offset), Out(np.prod(_oshape(vol, axis)), vol.dtype)
    L.check(L.lib().ivx_dev_lmip(L.DT[vol.dtype], d.ptr, *_dims(vol), axis, cdbl(tmin), cdbl(tmax), out.ptr, None), "dev_lmip")
    L.synchronize()
    d.close()
    return out.read(_oshape(vol, axis))


def dev_mida(L, vol, axis, wl, ww, offset=0):
    from invesalius3_amd.device import DeviceBuffer
    odt = np.dtype(np.int16) if vol.dtype == np.int16 else np.dtype(np.uint8)
    d, out, mm, st = Dev(vol, offset), Out(np.prod(_oshape(vol, axis)), odt), DeviceBuffer(64), _status()
    L.check(L.lib().ivx_dev_minmax_f32(L.DT[vol.dtype], d.ptr, _c64(vol.size), mm.ptr, None), "dev_minmax")
    L.check(L.lib().ivx_dev_mida(L.DT[vol.dtype], d.ptr, *_dims(vol), axis, cflt(wl), cflt(ww), mm.ptr, L.DT[odt], out.ptr, st.ptr, None),
            "dev_mida")
    _status_is_zero(L, st)
    got_mm = mm.download((2,), np.float32)
    assert got_mm[0] == np.float32(vol.min()) and got_mm[1] == np.float32(vol.max())
    mm.close()
    d.close()
    return out.read(_oshape(vol, axis))


def dev_fcm(L, vol, n, axis, offset=0):
    d, out, st = Dev(vol, offset), Out(np.prod(_oshape(vol, axis)), vol.dtype), _status()
    L.check(L.lib().ivx_dev_fcm_maxip(L.DT[vol.dtype], d.ptr, *_dims(vol), cflt(n), axis, out.ptr, st.ptr, None), "dev_fcm_maxip")
    _status_is_zero(L, st)
    d.close()
    return out.read(_oshape(vol, axis))


def _projection(kind, oracle, L, mips, vol, axis, p0, p1, offsets=(0,), what=""):
    """one volume through the oracle, the host form and the device form at each pointer offset"""
    odt = vol.dtype if kind == "lmip" or vol.dtype != np.float64 else np.dtype(np.uint8)
    want, got = np.zeros(_oshape(vol, axis), odt), np.zeros(_oshape(vol, axis), odt)
    if kind == "lmip":
        oracle.lmip(vol, axis, p0, p1, want)
        mips.lmip(vol, axis, p0, p1, got)
    else:
        oracle.mida(vol, axis, p0, p1, want)
        mips.mida(vol, axis, p0, p1, got)
    _same(got, want, what + " host form")
    for off in offsets:
        got = dev_lmip(L, vol, axis, p0, p1, off) if kind == "lmip" else dev_mida(L, vol, axis, p0, p1, off)
        _same(got, want, what + " device form, pointer + %d elements" % off)
    return want


def _windows(kind, dtype):
    return C.LMIP_WINDOWS[dtype] if kind == "lmip" else C.MIDA_WINDOWS[dtype]


def _rays(kind, npix, length, dtype):
    return (C.lmip_rays if kind == "lmip" else C.mida_rays)(npix, length, dtype)


# ---- MIDA and LMIP along axes 0 and 1: the block pipeline of k_rays_strided ---------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=["i16", "u8", "f64"])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("kind", ["lmip", "mida"])
def test_strided_walk_at_block_edges(ivxlib, oracle, kind, axis, dtype):
    """ray lengths 1, 2 and both sides of 16, 32 and 48 samples (every hand-over between the unguarded and the guarded loop),
    each with 63, 64, 65 and 257 rays: a wave short of a lane, a full wave, a wave and one lane, a second workgroup"""
    from invesalius3_amd import invesalius_rs as mips
    moved = 0
    for length in C.STRIDED_LENS:
        for npix in C.STRIDED_PIXELS:
            vol = C.place(_rays(kind, npix, length, dtype), axis)
            assert vol.shape[axis] == length and vol.size == npix * length
            for p0, p1 in _windows(kind, dtype):
                want = _projection(kind, oracle, ivxlib, mips, vol, axis, p0, p1, what="%s len %d, %d rays, window %r" % (kind, length, npix, (p0, p1)))
                moved += int(len(np.unique(want)) > 1)
    assert moved >= len(C.STRIDED_LENS) * len(C.STRIDED_PIXELS)  # (the pictures are not constant images)


# ---- MIDA and LMIP along axis 2: the staged chunks of k_rays_rows -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=["i16", "u8", "f64"])
@pytest.mark.parametrize("kind", ["lmip", "mida"])
def test_staged_walk_at_chunk_edges_aligned_and_not(ivxlib, oracle, kind, dtype):
    """rows of CH - 1, CH, CH + 1, 2 CH, 2 CH + 1 and CH + 16 bytes' worth of elements and one whose byte length is no multiple of 16; 1 to 257 rows (dead
    lanes in the last wave, a second workgroup); the device form a second time one element past an aligned address, where the
    16-byte loads are off for every length"""
    from invesalius3_amd import invesalius_rs as mips
    isz = dtype.itemsize
    for length in C.staged_lens(dtype):
        for nrays in C.STAGED_RAYS:
            assert C.staged_plan(length, isz, isz, nrays).vec_ok is False
            vol = C.place(_rays(kind, nrays, length, dtype), 2)
            assert vol.shape[2] == length and vol.shape[0] * vol.shape[1] == nrays
            for p0, p1 in _windows(kind, dtype)[:2]:
                _projection(kind, oracle, ivxlib, mips, vol, 2, p0, p1, offsets=(0, 1),
                            what="%s rows of %d, %d rays, window %r" % (kind, length, nrays, (p0, p1)))


# ---- early exit, built ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("case", C.EXIT_CASES, ids=C.ids(C.EXIT_CASES))
def test_rays_built_to_end_early(ivxlib, oracle, case, axis):
    """a wave whose 64 rays all end inside the first block next to a wave that runs to the end, and a wave in which one lane
    runs on alone: the vote must neither stop a living ray nor let a finished one pick up the samples behind its break"""
    from invesalius3_amd import invesalius_rs as mips
    vol = C.place(case.rays, axis)
    windows = [C.EXIT_LMIP_WINDOW, (-32768, 32767), (30000, 30100)] if case.kind == "lmip" else [C.EXIT_MIDA_WINDOW]
    for p0, p1 in windows:
        want = _projection(case.kind, oracle, ivxlib, mips, vol, axis, p0, p1, offsets=(0, 1) if axis == 2 else (0,),
                           what="%s axis %d window %r" % (case.name, axis, (p0, p1)))
    if case.kind == "lmip":  # (the last window: no sample enters it, no ray ends, every ray's answer is its largest sample)
        assert np.array_equal(want, case.rays.max(2))


# ---- the min / max pre-pass ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one-element-past"])
@pytest.mark.parametrize("dtype", C.DTYPES, ids=["i16", "u8", "f64"])
def test_minmax_with_the_extremes_in_body_tail_and_ends(ivxlib, dtype, offset):
    """n around one 16-byte vector, around one block, and past the cap of 2 048 blocks; the minimum and the maximum in turn at
    element 0, in the vector body, in the scalar tail and at the last element; against numpy's min / max cast to float32"""
    from invesalius3_amd.device import DeviceBuffer
    L = ivxlib
    lo, hi = C.MINMAX_ENDS[dtype]
    mm = DeviceBuffer(64)
    for n in C.minmax_sizes(dtype):
        base = C.minmax_base(n, dtype)
        trials = [("plain", base)]
        for spot, at in C.minmax_spots(n, dtype).items():
            for name, value in (("min", lo), ("max", hi)):
                a = base.copy()
                a[at] = value
                trials.append(("%s at %s (element %d)" % (name, spot, at), a))
        for what, a in trials:
            d = Dev(a, offset)
            mm.upload(np.full(2, np.nan, np.float32))
            L.check(L.lib().ivx_dev_minmax_f32(L.DT[dtype], d.ptr, _c64(n), mm.ptr, None), "dev_minmax")
            L.synchronize()
            got = mm.download((2,), np.float32)
            d.close()
            want = np.array([a.min(), a.max()]).astype(np.float32)
            assert np.array_equal(got, want), ("n = %d, %s" % (n, what), got, want)
    mm.close()


# ---- the contour MaxIP ---------------------------------------------------------------------------------------------------------------
def _fcm(ivxlib, oracle, case):
    from invesalius3_amd import invesalius_rs as mips
    vol = case.vol
    want = np.zeros(_oshape(vol, case.axis), np.int16)
    oracle.fast_countour_mip(vol, case.n, case.axis, 0, 0, 0, want)
    _same(dev_fcm(ivxlib, vol, case.n, case.axis, case.offset), want, case.name + " device form")
    got = np.zeros_like(want)
    mips.fast_countour_mip(vol, case.n, case.axis, 0, 0, 0, got)
    _same(got, want, case.name + " host form")
    return want


@pytest.mark.parametrize("case", C.VARIANT_CASES, ids=C.ids(C.VARIANT_CASES))
def test_contour_maxip_every_variant(ivxlib, oracle, case):
    """exponent 1 (fcm_lin_fold), 0.5 (bounds of the power), 2 and 3.3 (fcm_pow_fold), and 100 and 0: the exact walk, the exact rows
    and k_fcm_max_combine, which nothing else in the suite runs.  The oracle accepts both (test_ray_cases_host.py), so does the GPU."""
    want = _fcm(ivxlib, oracle, case)
    assert want.any()


@pytest.mark.parametrize("case", C.ROUTE_CASES, ids=C.ids(C.ROUTE_CASES))
def test_contour_maxip_route_switches(ivxlib, oracle, case):
    """rows of one chunk, two chunks and 65 chunks (a lane's second round in k_fcm_max_rows), ragged rows and an unaligned pointer
    (both through the materialised contour volume); the volumes carry gradients on their first and last rows and columns,
    where the neighbours om / op / left / right are clamped"""
    _fcm(ivxlib, oracle, case)


@pytest.mark.parametrize("case", C.FORCED_OPEN_CASES, ids=C.ids(C.FORCED_OPEN_CASES))
def test_contour_maxip_pixels_only_the_exact_pass_can_settle(ivxlib, oracle, case):
    """every interior pixel's maximum is an exact integer strictly inside its bounds: k_fcm_max_decide must leave it open with the
    right segment bits and k_fcm_fix must write the value -- a decided pixel would be one too low, a lost segment too
    (test_ray_cases_host.py shows both on the oracle's contour volume).  Rays of 64, 75, 1 024 and 1 030 voxels: 2 even, 2 ragged, 32
    even and 32 ragged segments, the maximum in the first, in the last, at the borders and behind bit 31."""
    want = _fcm(ivxlib, oracle, case)
    assert (want[C.interior(want.shape)] == case.value).all()
