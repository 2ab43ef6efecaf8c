"""Resident host arrays: declare once that a numpy array is the project's image (`Slice.matrix`) or a mask's matrix, and
every entry point of this package that is handed that array -- or any view of it -- finds the bytes already in HBM
(the registry lives under the library's copy helpers, include/ivx.h "resident host arrays").

    img = resident.bind(slice_matrix)        # one upload
    ... any number of calls on slice_matrix, slice_matrix[a:b], mask.matrix[1:, 1:, 1:] ...
    slice_matrix[5] = something              # whoever writes the array with numpy ...
    img.touch(slice_matrix[5:6])             # ... says so: exactly these bytes are uploaded again at the next use
    img.release()                            # or `with resident.bind(a) as r:`, or drop the last reference

What the library itself writes into a bound array (a thresholded mask, a flood's result) goes to the host AND into the
mirror; nothing has to be touched after it.  `set_check(True)` (or IVX_RESIDENT_CHECK=1) makes every use compare the host
bytes with the mirror first and raise `StaleError` on a forgotten touch -- at the price of the upload the binding saves."""
from __future__ import annotations

import ctypes
import weakref

import numpy as np

from . import _lib as L

_STAT_NAMES = ("hits", "hit_bytes", "refreshes", "refresh_bytes", "write_throughs", "write_through_bytes", "invalidations",
               "generation")
_live = weakref.WeakValueDictionary()  # (address, nbytes) of a bound allocation -> its Resident
_kept = {}  # the bindings the package made itself (bind_zeros(keep=True)): held until released


def _byte_bounds(a: np.ndarray):
    """[lo, hi) of the bytes a view can reach (numpy's byte_bounds; an empty view reaches nothing)"""
    lo = hi = a.ctypes.data
    for n, s in zip(a.shape, a.strides):
        if n == 0:
            return lo, lo
        if s < 0:
            lo += (n - 1) * s
        else:
            hi += (n - 1) * s
    return lo, hi + a.itemsize


def _root(a: np.ndarray) -> np.ndarray:
    """the array that owns the allocation `a` is a view of (the end of the .base chain: a plain array, or the np.memmap)"""
    while isinstance(a.base, np.ndarray):
        a = a.base
    return a


def _release_handle(handle: int):
    try:
        L.lib().ivx_host_release(handle)
    except Exception:
        pass


class Resident:
    """One registered allocation.  Holds a strong reference to the array, so the memory cannot be freed and handed out
    again while the library still answers for its address."""

    def __init__(self, root: np.ndarray, handle: int, lo: int, nbytes: int):
        self.array, self.handle, self.address, self.nbytes = root, int(handle), int(lo), int(nbytes)
        self._released = False
        self._fin = weakref.finalize(self, _release_handle, self.handle)

    def touch(self, view_or_slice=None):
        """The host wrote the array: all of it (no argument), a view of it, or `array[view_or_slice]`.  The bytes between
        the view's first and last byte are uploaded again at the next use."""
        lib = L.lib()
        if view_or_slice is None:
            L.check(lib.ivx_host_touch(self.handle), "resident.touch")
            return
        v = view_or_slice if isinstance(view_or_slice, np.ndarray) else self.array[view_or_slice]
        lo, hi = _byte_bounds(v)
        if hi == lo:
            return
        if lo < self.address or hi > self.address + self.nbytes:
            raise TypeError("resident.touch: not a view of the bound array")
        L.check(lib.ivx_host_touch_range(self.handle, lo - self.address, hi - lo), "resident.touch")

    def stats(self) -> dict:
        out = (ctypes.c_uint64 * 8)()
        L.check(L.lib().ivx_host_stats(self.handle, out), "resident.stats")
        return dict(zip(_STAT_NAMES, (int(v) for v in out)))

    def release(self):
        """Free the mirror.  The handle is dead afterwards: touch() and stats() raise."""
        if self._released:
            return
        self._released = True
        self._fin.detach()
        _live.pop((self.address, self.nbytes), None)
        _kept.pop((self.address, self.nbytes), None)
        L.check(L.lib().ivx_host_release(self.handle), "resident.release")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
        return False


def bind(array: np.ndarray) -> Resident:
    """Register the allocation behind `array` (the array itself, or what it is a view of) on the current device and
    upload it once.  Binding the same allocation again returns the live `Resident`; an allocation that overlaps another
    bound one is a TypeError, a mirror that does not fit a MemoryError (the array then simply stays unregistered)."""
    if not isinstance(array, np.ndarray):
        raise TypeError("resident.bind: a numpy array (or np.memmap)")
    L.require_device()
    root = _root(array)
    lo, hi = _byte_bounds(root)
    if hi == lo:
        raise TypeError("resident.bind: empty array")
    live = _live.get((lo, hi - lo))
    if live is not None and not live._released:
        return live
    h = ctypes.c_uint64(0)
    L.check(L.lib().ivx_host_register(ctypes.c_void_p(lo), hi - lo, ctypes.byref(h)), "resident.bind")
    r = Resident(root, h.value, lo, hi - lo)
    _live[(lo, hi - lo)] = r
    return r


def bind_zeros(array: np.ndarray, keep: bool = False) -> Resident:
    """`bind` for an array of zeros (``np.zeros``) that a library call is about to fill: the mirror starts as zeros too and
    nothing is uploaded (ivx_host_register_zero).  The caller answers for the zeros.  `keep`: the package made the binding
    on the caller's behalf (the new arrays of slice_.swap_volume_axes) and holds it until ``find(array).release()``."""
    if not isinstance(array, np.ndarray):
        raise TypeError("resident.bind_zeros: a numpy array")
    L.require_device()
    root = _root(array)
    lo, hi = _byte_bounds(root)
    if hi == lo:
        raise TypeError("resident.bind_zeros: empty array")
    h = ctypes.c_uint64(0)
    L.check(L.lib().ivx_host_register_zero(ctypes.c_void_p(lo), hi - lo, ctypes.byref(h)), "resident.bind_zeros")
    r = Resident(root, h.value, lo, hi - lo)
    _live[(lo, hi - lo)] = r
    if keep:
        _kept[(lo, hi - lo)] = r
    return r


def find(array: np.ndarray):
    """the live `Resident` whose allocation holds all of `array`, or None (what the package's own numpy writers ask)"""
    lo, hi = _byte_bounds(array)
    for r in list(_live.values()):
        if not r._released and r.address <= lo and hi <= r.address + r.nbytes:
            return r
    return None


def touch(array: np.ndarray):
    """`find(array).touch(array)` when the array is bound; nothing otherwise"""
    if _live:
        r = find(array)
        if r is not None:
            r.touch(array)


def count() -> int:
    """registrations alive in the library"""
    n = ctypes.c_uint64(0)
    L.check(L.lib().ivx_host_count(ctypes.byref(n)), "resident.count")
    return int(n.value)


def transfer_stats() -> dict:
    """bytes the library's copy helpers have moved since the process started: host -> device, device -> host, host -> device
    for the stale check alone (not part of the first), and served device -> device from mirrors"""
    out = (ctypes.c_uint64 * 4)()
    L.check(L.lib().ivx_transfer_stats(out), "resident.transfer_stats")
    return dict(zip(("h2d_bytes", "d2h_bytes", "check_h2d_bytes", "served_bytes"), (int(v) for v in out)))


def set_check(on: bool):
    """the stale check (also IVX_RESIDENT_CHECK=1): every use of a bound array compares host and mirror first"""
    L.check(L.lib().ivx_host_set_check(int(bool(on))), "resident.set_check")
