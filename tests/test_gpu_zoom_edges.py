"""The order-2 zoom (csrc/k_zoom.hip) where test_gpu_zoom.py does not reach: the end planes scipy zeroes (ZoomTab.zero), the
clamp to the type's range, axes of one and two samples, one-sample and empty outputs, factors of 1 and above, lines whose pole
power underflows, counts at the 256-lane block edges, the device form with its scratch layout on two streams, its argument
checks, and the Python wrapper's edges.  Cases come from _zoom_cases.py; test_zoom_cases_host.py proves without a device that
each case is where its name says.  The reference is live scipy and every comparison is np.array_equal: the claim is bit
equality, so there is no tolerance anywhere in this file."""
import ctypes
import functools
import os
import tempfile

import numpy as np
import pytest
from scipy import ndimage

import _zoom_cases as C

pytestmark = pytest.mark.gpu

cint = ctypes.c_int
GUARD, SENTINEL = 256, 0xA5
TAB_BYTES = 40  # sizeof(ZoomTab): int32 idx[3], int32 zero, double w[3]


@functools.lru_cache(maxsize=None)
def _scipy(name):
    c = C.by_name(name)
    want = ndimage.zoom(c.array, c.factor, c.array.dtype, order=2)
    want.setflags(write=False)
    return want


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d voxels differ from scipy, first at %s: got %d, scipy %d"
                             % (what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- every case through the wrapper ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.ids(C.ALL_CASES))
def test_zoom_case_equals_scipy(ivxlib, case):
    from invesalius3_amd import surface_process as sp
    got = sp.resize_image_array(case.array, case.factor)
    _same(got, _scipy(case.name), case.name)


@pytest.mark.parametrize("case", C.ZERO_END_CASES, ids=C.ids(C.ZERO_END_CASES))
def test_zeroed_end_plane_is_zero_and_nothing_else_is(ivxlib, case):
    """ZoomTab.zero: the last output plane along each named axis is all zero, as scipy's is, and along every other axis it is
    not (a near miss must not take the branch)"""
    from invesalius3_amd import surface_process as sp
    got = sp.resize_image_array(case.array, case.factor)
    for ax in range(3):
        last = np.take(got, -1, axis=ax)
        if ax in case.zero_axes:
            assert not last.any(), ("the zeroed-end branch (ZoomTab.zero) was not taken along axis %d: %d of %d voxels of the "
                                    "end plane are not zero" % (ax, int(np.count_nonzero(last)), last.size))
            assert np.take(got, -2, axis=ax).any(), "the plane before the zeroed end of axis %d is zero as well" % ax
        else:
            assert last.any(), "the zeroed-end branch was taken along axis %d, where the last coordinate does not overshoot" % ax


@pytest.mark.parametrize("case", C.CLAMP_CASES, ids=C.ids(C.CLAMP_CASES))
def test_clamped_voxels_sit_on_the_limit(ivxlib, case):
    """where scipy's float64 result passes the type's range by more than 0.5 the output is the limit itself, not a wrapped value"""
    from invesalius3_amd import surface_process as sp
    lo, hi = C.LIMITS[case.array.dtype]
    f = ndimage.zoom(case.array, case.factor, np.float64, order=2)
    got = sp.resize_image_array(case.array, case.factor)
    above, below = f > hi + 0.5, f < lo - 0.5
    assert bool(above.any()) == ("hi" in case.sides) and bool(below.any()) == ("lo" in case.sides)
    assert (got[above] == hi).all(), "the clamp to the upper limit: %d voxels wrapped" % int((got[above] != hi).sum())
    assert (got[below] == lo).all(), "the clamp to the lower limit: %d voxels wrapped" % int((got[below] != lo).sum())


# ---- the device form ------------------------------------------------------------------------------------------------------------
class Guarded:
    """a device block of exactly `nbytes` usable bytes at a 256-byte aligned address, with sentinel bytes on both sides; the
    region itself starts out as sentinels too unless `init` is given"""

    def __init__(self, nbytes, init=None):
        from invesalius3_amd.device import DeviceBuffer
        self.lo, self.n = GUARD, int(nbytes)
        self.total = (self.lo + self.n + GUARD + 15) // 16 * 16
        host = np.full(self.total, SENTINEL, np.uint8)
        if init is not None:
            raw = np.ascontiguousarray(init).reshape(-1).view(np.uint8)
            assert raw.size == self.n
            host[self.lo:self.lo + self.n] = raw
        self.buf = DeviceBuffer(self.total)
        self.buf.upload(host)
        self.ptr = self.buf.at(self.lo)
        assert self.ptr.value % 256 == 0

    def raw(self):
        return self.buf.download((self.total,), np.uint8)

    def guards_intact(self):
        host = self.raw()
        return bool((host[:self.lo] == SENTINEL).all() and (host[self.lo + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.raw() == SENTINEL).all())

    def read(self, shape, dtype):
        host = self.raw()
        return host[self.lo:self.lo + self.n].copy().view(dtype).reshape(shape)


def _scratch_bytes(L, ishape, oshape):
    nb = ctypes.c_size_t(0)
    L.check(L.lib().ivx_zoom_scratch_bytes(L.i64(ishape), L.i64(oshape), ctypes.byref(nb)), "zoom_scratch_bytes")
    return nb.value


def _dev_zoom(L, a, oshape, scratch, stream):
    """ivx_dev_zoom_order2 of the host array `a` through guarded device buffers -> (result, output guards intact?)"""
    d_in = Guarded(a.nbytes, a)
    d_out = Guarded(int(np.prod(oshape)) * a.itemsize)
    L.check(L.lib().ivx_dev_zoom_order2(cint(L.DT[a.dtype]), d_in.ptr, L.i64(a.shape), d_out.ptr, L.i64(oshape), scratch.ptr, stream),
            "dev_zoom")
    L.check(L.lib().ivx_stream_synchronize(stream))
    assert d_in.guards_intact() and np.array_equal(d_in.read(a.shape, a.dtype), a), "the input was written"
    return d_out.read(oshape, a.dtype), d_out.guards_intact()


def test_scratch_bytes_is_the_documented_layout(ivxlib):
    """n float64 coefficients, the tables from the next 256-byte boundary: n * 8 + 256 + (oz + oy + ox) * sizeof(ZoomTab)"""
    for ishape, oshape in (((28, 30, 7), (14, 15, 4)), ((1, 1, 1), (1, 1, 1)), ((4, 8, 8), (2, 4, 4)), ((9, 10, 11), (18, 20, 22))):
        n = int(np.prod(ishape))
        nb = _scratch_bytes(ivxlib, ishape, oshape)
        assert nb == n * 8 + 256 + sum(oshape) * TAB_BYTES
        assert (n * 8 + 255) // 256 * 256 + sum(oshape) * TAB_BYTES <= nb  # the tables the device form places fit


@pytest.mark.parametrize("own_stream", [False, True], ids=["null-stream", "volume-stream"])
@pytest.mark.parametrize("first,second", [("zero-ax01-28x30-i16", "clamp-u8-checker-cell2-3over2"),
                                          ("clamp-u8-ends-draw-x2", "zero-ax0-28-i16")])
def test_device_form_scratch_guards_streams_and_reuse(ivxlib, first, second, own_stream):
    """input, output and scratch in device buffers; the scratch has exactly ivx_zoom_scratch_bytes bytes between sentinels;
    then a second, different shape goes through the same scratch with the first run's coefficients and tables still in it"""
    from invesalius3_amd.device import DeviceVolume
    L = ivxlib
    c1, c2 = C.by_name(first), C.by_name(second)
    o1, o2 = C.out_shape(c1.array.shape, c1.factor), C.out_shape(c2.array.shape, c2.factor)
    nb1, nb2 = _scratch_bytes(L, c1.array.shape, o1), _scratch_bytes(L, c2.array.shape, o2)
    assert nb2 < nb1 and c2.array.shape != c1.array.shape
    # the second run's tables land inside what the first run's coefficients occupied
    assert (c2.array.size * 8 + 255) // 256 * 256 < c1.array.size * 8
    vol = DeviceVolume(np.zeros((2, 3, 64), np.int16)) if own_stream else None
    try:
        stream = vol.stream if own_stream else None
        scratch = Guarded(nb1)
        got, out_ok = _dev_zoom(L, c1.array, o1, scratch, stream)
        assert out_ok, "bytes outside the output were written"
        assert scratch.guards_intact(), "bytes outside the %d bytes of ivx_zoom_scratch_bytes were written" % nb1
        _same(got, _scipy(first), first)
        if c1.zero_axes:
            for ax in c1.zero_axes:
                assert not np.take(got, -1, axis=ax).any(), "ZoomTab.zero along axis %d" % ax
        stale = scratch.read((nb1,), np.uint8)
        assert (stale[:c1.array.size * 8] != SENTINEL).any()  # the first run did leave its coefficients behind
        got2, out_ok = _dev_zoom(L, c2.array, o2, scratch, stream)
        assert out_ok and scratch.guards_intact()
        _same(got2, _scipy(second), second + " on stale scratch")
    finally:
        if vol is not None:
            vol.close()


def _bad_call(L, dtype=None, ishape=(4, 5, 6), oshape=(2, 2, 3), null=None):
    """one call that must be refused: -> the buffers, which must still hold nothing but sentinels"""
    bufs = {"in": Guarded(240), "out": Guarded(24), "scratch": Guarded(_scratch_bytes(L, (4, 5, 6), (2, 2, 3)))}
    p = {k: (None if k == null else b.ptr) for k, b in bufs.items()}
    rc = L.lib().ivx_dev_zoom_order2(cint(L.I16 if dtype is None else dtype), p["in"], L.i64(ishape), p["out"], L.i64(oshape),
                                     p["scratch"], None)
    assert rc == L.IVX_EINVAL
    with pytest.raises(TypeError, match="zoom"):
        L.check(rc, "dev_zoom")
    L.synchronize()
    for k, b in bufs.items():
        assert b.untouched(), "a refused call wrote to its %s buffer" % k


@pytest.mark.parametrize("dtype", ["F64", "U16", "F32", "I32", "I64", "I8", 99, -1])
def test_device_form_refuses_other_dtypes(ivxlib, dtype):
    _bad_call(ivxlib, dtype=getattr(ivxlib, dtype) if isinstance(dtype, str) else dtype)


@pytest.mark.parametrize("which,axis", [(w, a) for w in ("ishape", "oshape") for a in range(3)])
def test_device_form_refuses_a_zero_extent(ivxlib, which, axis):
    shapes = {"ishape": [4, 5, 6], "oshape": [2, 2, 3]}
    shapes[which][axis] = 0
    _bad_call(ivxlib, **{k: tuple(v) for k, v in shapes.items()})


@pytest.mark.parametrize("null", ["in", "out", "scratch"])
def test_device_form_refuses_a_null_pointer(ivxlib, null):
    _bad_call(ivxlib, null=null)


# ---- the wrapper's Python edges ---------------------------------------------------------------------------------------------------
def test_wrapper_takes_a_transposed_view_and_a_read_only_memmap(ivxlib, tmp_path):
    from invesalius3_amd import surface_process as sp
    base = C.by_name("zero-ax2-32-i16").array                      # (5, 6, 32)
    view = base.transpose(2, 0, 1)                                 # (32, 5, 6): zeroed end along axis 0
    assert not view.flags["C_CONTIGUOUS"] and C.zeroed_axes(view.shape, 0.5) == (0,)
    dense = np.ascontiguousarray(view)
    want = ndimage.zoom(dense, 0.5, dense.dtype, order=2)
    _same(sp.resize_image_array(dense, 0.5), want, "dense copy")
    _same(sp.resize_image_array(view, 0.5), want, "transposed view")
    for a in (dense, C.by_name("clamp-u8-ends-draw-half").array):
        name = str(tmp_path / ("vol_%s.dat" % a.dtype.name))
        np.memmap(name, dtype=a.dtype, mode="w+", shape=a.shape)[:] = a
        mm = np.memmap(name, dtype=a.dtype, mode="r", shape=a.shape)
        assert not mm.flags["WRITEABLE"]
        _same(sp.resize_image_array(mm, 0.5), ndimage.zoom(a, 0.5, a.dtype, order=2), "read-only memmap")
        assert np.array_equal(mm, a)


def test_wrapper_refuses_float32_and_two_dimensions(ivxlib):
    from invesalius3_amd import surface_process as sp
    with pytest.raises(TypeError):
        sp.resize_image_array(np.zeros((4, 5, 6), np.float32), 0.5)
    with pytest.raises(TypeError):
        sp.resize_image_array(np.zeros((8, 9), np.int16), 0.5)
    with pytest.raises(TypeError):
        sp.resize_image_array(np.zeros((2, 3, 4, 5), np.uint8), 0.5)


def test_wrapper_as_mmap_on_an_empty_output(ivxlib):
    """(4, 1, 5) at 1/2 -> (2, 0, 2).  The reference's resize_image_array makes the same np.memmap(fname, shape, dtype, "w+")
    call on a fresh temporary file, so what numpy does with an empty shape decides: numpy 2 maps it (an empty memmap comes
    back); an older numpy that raises ValueError there makes the reference raise it too.  The wrapper must do the same."""
    from invesalius3_amd import surface_process as sp
    for name in ("short-empty-4x1x5-half-i16", "short-empty-4x1x5-half-u8"):
        a = C.by_name(name).array
        fd, fname = tempfile.mkstemp(suffix="_probe")
        os.close(fd)
        try:
            np.memmap(fname, shape=(2, 0, 2), dtype=a.dtype, mode="w+")
            numpy_error = None
        except (ValueError, OSError) as e:
            numpy_error = type(e)
        finally:
            os.remove(fname)
        if numpy_error is not None:
            with pytest.raises(numpy_error):
                sp.resize_image_array(a, 0.5, as_mmap=True)
            continue
        got = sp.resize_image_array(a, 0.5, as_mmap=True)
        try:
            assert isinstance(got, np.memmap) and got.shape == (2, 0, 2) and got.dtype == a.dtype
            assert os.path.exists(got.filename) and got.filename.endswith("_resized")
        finally:
            os.remove(got.filename)
    # and a non-empty one-sample output comes back through the file intact
    c = C.by_name("short-in2-all-2x2x2-half-i16")
    got = sp.resize_image_array(c.array, 0.5, as_mmap=True)
    try:
        assert isinstance(got, np.memmap)
        _same(np.asarray(got), _scipy(c.name), c.name)
    finally:
        os.remove(got.filename)
