"""Resident-volume pipeline: upload the int16 volume once, then threshold -> region growing -> marching cubes ->
projections all run on buffers that stay in HBM (at one GPU the PCIe staging of the host-level
entry points dominates; the GUI data layer keeps `Slice.matrix` for the whole session, so does this class).

Everything here is a thin ctypes veneer over the `ivx_dev_*` C ABI (include/ivx.h); kernels are launched on one
HIP stream owned by the object, and `Timer` records HIP events on that same stream.
"""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional

import numpy as np

from . import _lib as L
from .mc_ride import RideBook


class _MaskLevels(NamedTuple):
    """a uint8 mask whose bytes are known: `v_in` inside the inside plane, `v_sel` where the plane `sel` has a bit.  Without a
    second level `sel` is None (NULL for the kernels that accept it) and `v_sel == v_in`."""
    v_in: float
    sel: Optional[ctypes.c_void_p]
    v_sel: float

    @property
    def has_second(self):
        return self.sel is not None


class DeviceBuffer:
    """A hipMalloc'ed block (freed on close / GC)."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        L.check(L.lib().ivx_malloc(ctypes.byref(p), ctypes.c_size_t(max(self.nbytes, 16))), "ivx_malloc")
        self.ptr = p

    def upload(self, a: np.ndarray):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        L.check(L.lib().ivx_memcpy_h2d(self.ptr, L.ptr(a), ctypes.c_size_t(a.nbytes)))

    def upload_view(self, a: np.ndarray):
        """upload() of a view as it stands -- `matrix[1:, 1:, 1:]`, a slab, a reversed or stepped axis -- without the host
        copy np.ascontiguousarray would make: the library walks the strides (ivx_upload_strided), and a view of an array
        bound with resident.bind comes out of its mirror in HBM.  More than three axes, or items that are not 1 / 2 / 4 / 8
        bytes, take the copy."""
        a = np.asarray(a)
        if a.ndim > 3 or a.itemsize not in (1, 2, 4, 8) or a.ndim == 0:
            return self.upload(a)
        assert a.nbytes <= self.nbytes
        pad = 3 - a.ndim  # (leading axes of length 1, with the stride a dense array would have there)
        L.check(L.lib().ivx_upload_strided(self.ptr, L.ptr(a), L.i64((1,) * pad + a.shape),
                                           L.i64((a.strides[0] * a.shape[0],) * pad + a.strides), a.itemsize), "upload_view")

    def download_view(self, out: np.ndarray):
        """the block's leading bytes into the view `out` (same rules as upload_view); the bytes of `out`'s parent between
        the view's elements are left as they are"""
        if out.ndim > 3 or out.itemsize not in (1, 2, 4, 8) or out.ndim == 0:
            out[...] = self.download(out.shape, out.dtype)
            return out
        assert out.nbytes <= self.nbytes
        pad = 3 - out.ndim
        L.check(L.lib().ivx_download_strided(L.ptr(out), L.i64((1,) * pad + out.shape),
                                             L.i64((out.strides[0] * out.shape[0],) * pad + out.strides), self.ptr, out.itemsize),
                "download_view")
        return out

    def download(self, shape, dtype, out: np.ndarray | None = None) -> np.ndarray:
        """`out`: a C-contiguous array with room for the result (e.g. `_lib.pinned_empty`); a view of it is returned"""
        if out is None:
            out = np.empty(shape, dtype)
        else:
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            assert out.flags["C_CONTIGUOUS"] and out.nbytes >= n
            out = out.reshape(-1).view(np.uint8)[:n].view(dtype).reshape(shape)
        assert out.nbytes <= self.nbytes
        L.check(L.lib().ivx_memcpy_d2h(L.ptr(out), self.ptr, ctypes.c_size_t(out.nbytes)))
        return out

    def zero(self, stream=None, nbytes=None):
        L.check(L.lib().ivx_memset(self.ptr, 0, ctypes.c_size_t(self.nbytes if nbytes is None else nbytes), stream))

    def at(self, offset_bytes: int) -> ctypes.c_void_p:
        return ctypes.c_void_p(self.ptr.value + int(offset_bytes))

    def close(self):
        if self.ptr is not None and self.ptr.value:
            L.lib().ivx_free(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrackedBuffer(DeviceBuffer):
    """A DeviceBuffer that reports every access from outside its owner (`ptr`, and through it upload / zero / at):
    the owner then stops trusting what it derived from the contents (DeviceVolume's inside-bit plane of the mask,
    the "out_mask is all zero" note).  The owner's own kernels use `raw`.  `on_read` is called before a download: an owner
    that has deferred writing the bytes (DeviceVolume's mask) writes them then, and keeps its notes."""

    def __init__(self, nbytes: int, on_touch, on_read=None):
        self._on_touch = self._on_read = None
        super().__init__(nbytes)
        self._on_touch, self._on_read = on_touch, on_read

    @property
    def ptr(self):
        if self._on_touch is not None:
            self._on_touch()
        return self._p

    @ptr.setter
    def ptr(self, v):
        self._p = v

    @property
    def raw(self):
        return self._p

    def download(self, shape, dtype, out=None) -> np.ndarray:  # reading changes nothing
        if self._on_read is not None:
            self._on_read()
        if out is None:
            out = np.empty(shape, dtype)
        else:
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            assert out.flags["C_CONTIGUOUS"] and out.nbytes >= n
            out = out.reshape(-1).view(np.uint8)[:n].view(dtype).reshape(shape)
        assert out.nbytes <= self.nbytes
        L.check(L.lib().ivx_memcpy_d2h(L.ptr(out), self._p, ctypes.c_size_t(out.nbytes)))
        return out

    def raw_at(self, offset_bytes: int) -> ctypes.c_void_p:
        return ctypes.c_void_p(self._p.value + int(offset_bytes))


class Timer:
    """HIP events on the pipeline's stream: `with t.span('name'):` accumulates milliseconds per name."""

    def __init__(self, stream):
        self.stream = stream
        self.spans = []  # (name, ev0, ev1)
        self._pool = []
        # Names to record (None = all).  A recorded event is a barrier packet in the stream: ~4 us of idle GPU each, so
        # a caller timing whole steps by the wall clock brackets only what it needs.
        self.only = None

    class _Off:
        def __enter__(self):
            return None

        def __exit__(self, *a):
            return False

    _OFF = _Off()

    def _ev(self):
        if self._pool:
            return self._pool.pop()
        e = ctypes.c_void_p()
        L.check(L.lib().ivx_event_create(ctypes.byref(e)))
        return e

    class _Span:
        def __init__(self, t, name):
            self.t, self.name = t, name

        def __enter__(self):
            self.e0 = self.t._ev()
            L.check(L.lib().ivx_event_record(self.e0, self.t.stream))

        def __exit__(self, *a):
            e1 = self.t._ev()
            L.check(L.lib().ivx_event_record(e1, self.t.stream))
            self.t.spans.append((self.name, self.e0, e1))

    def records(self, name) -> bool:
        return self.only is None or name in self.only

    def span(self, name):
        if not self.records(name):
            return Timer._OFF
        return Timer._Span(self, name)

    def collect(self) -> dict:
        """-> {name: [ms, ...]} and recycles the events."""
        out = {}
        for name, e0, e1 in self.spans:
            ms = ctypes.c_float(0)
            L.check(L.lib().ivx_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
            out.setdefault(name, []).append(ms.value)
            self._pool += [e0, e1]
        self.spans = []
        return out


class DeviceVolume:
    """An int16 (dz, dy, dx) volume resident in HBM with its dense uint8 mask and the work buffers of the path."""

    def __init__(self, image: np.ndarray | None = None, shape=None, spacing=(1.0, 1.0, 1.0), device: int | None = None):
        L.require_device()
        if device is not None:
            L.set_device(device)
        if image is not None:
            if image.dtype != np.int16 or image.ndim != 3:
                raise TypeError("image must be a 3-D int16 array")
            shape = image.shape
        self.shape = tuple(int(s) for s in shape)
        self.dz, self.dy, self.dx = self.shape
        self.n = self.dz * self.dy * self.dx
        self.spacing = tuple(float(s) for s in spacing)
        s = ctypes.c_void_p()
        L.check(L.lib().ivx_stream_create(ctypes.byref(s)))
        self.stream = s
        self.timer = Timer(self.stream)
        # Derived state the pipeline keeps about its buffers (see `threshold`): any access to these three buffers from
        # outside this class's own kernels (their .ptr / upload / zero) drops the corresponding note.
        self._mbits_valid = False   # self._mbits == (mask >= 127), the inside plane marching cubes needs at iso 127
        self._mbits_range = None    # (lo, hi) while additionally _mbits == (lo <= image <= hi)
        # (v_in, v_sel | None) while the mask's BYTES are known: 0 outside _mbits, v_sel where self.reached has a bit (if
        # given), v_in elsewhere inside -- marching cubes then needs no voxel at all (ivx_dev_mc_emit_levels)
        self._mask_levels = None
        self._out_bytes_zero = False  # the BYTES of out_mask are all zero
        self._mc_params_cache = {}
        # surface_prefetch: marching cubes' count + list queued on a second stream under the region growing
        self._stream2 = None
        self._sync_events = []
        self._prefetch = None     # (params, z0, capacity, plane version) of the outstanding prefetch
        self._gate = None         # device word the flood opens once its busy rounds are over
        self._gate_epoch = 0
        self._gate_armed = False  # armed and no flood has run since (so nobody will open it)
        self._mbits_version = 0   # bumped whenever the inside plane is rewritten
        self._out_pending = None      # fill value of a deferred `out_mask[reached] = fill` (self.reached still holds it)
        # the mask's bytes in HBM are stale: they are what _mask_levels says of _mbits (and self.reached), not yet written
        self._mask_pending = False
        self._defer_pays = True       # the last fused threshold's bytes were (or could have been) written by a flood's apply
        self._fuse = os.environ.get("IVX_NO_FUSE", "") == ""
        self._apply_levels = os.environ.get("IVX_APPLY_LEVELS", "1") != "0"  # (A/B: mask[reached] = v from the bit planes alone)
        self._use_ranges = os.environ.get("IVX_RANGES", "1") != "0"  # (A/B: threshold / candidates from the per-word records)
        self._mask_defer = os.environ.get("IVX_MASK_DEFER", "1") != "0"  # (A/B: plane-only threshold, mask bytes written later)
        self._select = os.environ.get("IVX_FLOOD_SELECT", "1") != "0"  # (A/B: the flood's write queued by the flood's own call)
        # marching cubes' count in the launch of the flood's mask write (mc_ride.py has the rules); IVX_MC_RIDE=0: never
        self._ride = RideBook(os.environ.get("IVX_MC_RIDE", "1") != "0")
        self._look_ahead = -1  # ivx_dev_flood_grow_select's look-ahead; negative = the library's default (tests drive 0 .. 3)
        # (min, max) of every 64-voxel x-word of the image (ivx_dev_image_ranges_i16): written by the first fused threshold
        # after the image's bytes changed, read by every later one.  Dropped with the image (_image_touched), like _range_valid.
        self._ranges = None
        self._ranges_valid = False
        self.image = TrackedBuffer(self.n * 2, self._image_touched)
        self.mask = TrackedBuffer(self.n, self._mask_touched, self._mask_read)  # dense interior of mask.matrix[1:,1:,1:]
        self.out_mask = TrackedBuffer(self.n, self._out_touched)    # region-growing `out` (styles.py:3190)
        if image is not None:
            self.image.upload_view(image)
        self.mask.zero(self.stream)
        self.zero_out_mask()
        # region growing bit planes + tile work-list
        self.plan = L.FloodPlan(self.dz, self.dy, self.dx, (self.dx + 63) // 64, 0)
        nb, ns = ctypes.c_size_t(0), ctypes.c_size_t(0)
        L.check(L.lib().ivx_flood_bits_bytes(ctypes.byref(self.plan), ctypes.byref(nb)))
        L.check(L.lib().ivx_flood_scratch_bytes(ctypes.byref(self.plan), ctypes.byref(ns)))
        self.cand = DeviceBuffer(nb.value)
        self.reached = DeviceBuffer(nb.value)
        self._mbits = DeviceBuffer(nb.value)
        self._plane_words = nb.value // 8
        self.flood_scratch = DeviceBuffer(ns.value)
        self._mc_scratch = None
        self._tris = None
        self._verts = None
        self._faces = None
        self._range_buf = None
        self._range_valid = False
        self.sync()

    # -- plumbing -------------------------------------------------------------------------------------
    def _image_touched(self):
        self._mbits_range = None
        self._range_valid = False
        self._ranges_valid = False
        self._drop_volren()

    def _mask_touched(self):
        self._mask_read()
        self._mp_cells_valid = False
        self._mbits_valid = False
        self._mbits_range = None
        self._mask_levels = None
        self._mbits_version += 1

    # Two buffers whose bytes follow from bit planes are written when somebody needs them, not when they become known.
    #
    # mask: a fused threshold writes the inside plane only and leaves `_mask_pending`: the bytes are 255 * _mbits (in general
    # what _mask_levels says of _mbits and self.reached), and the 134 MB of a 512^3 mask are stored once per step, by the pass
    # that has to write mask bytes anyway -- `mask[reached] = v` of the region growing (ivx_dev_mask_from_planes in
    # _apply_reached) -- or by _materialize_mask().  No public method but surface_prefetch returns with the note set unless
    # it is a threshold itself: every other one writes all bytes or begins with _materialize_mask(), and so does everything
    # that reads or hands out the bytes (mask.ptr, mask.download, mask_bytes()).
    # Deferring pays only where the region growing's pass consumes the note: a pass of its own for the bytes costs more than
    # the fused kernel's stores once the volume is past the Infinity Cache (2048^3: 1.25 + 2.15 ms against 2.97 ms).  So
    # `_defer_pays` follows the last threshold's fate -- off when its bytes needed _materialize_mask(), on when a flood's
    # apply took them (or would have) -- and a threshold that is not expected to pay runs the fused kernel.
    def _materialize_mask(self):
        if self._mask_pending:
            self._defer_pays = False
            lv = self._mask_levels
            sel = self.reached.ptr if lv[1] is not None else None
            with self.timer.span("mask_bytes"):
                L.check(L.lib().ivx_dev_mask_from_planes(ctypes.byref(self.plan), self._mbits.ptr, sel, self.mask.raw, int(lv[0]),
                                                         int(lv[0] if lv[1] is None else lv[1]), self.stream), "mask_from_planes")
            self._mask_pending = False

    def _mask_read(self):
        """somebody outside the pipeline's stream is about to look at the mask's bytes (or to write some of them)"""
        if self._mask_pending:
            self._materialize_mask()
            self.sync()  # (uploads and downloads do not run on self.stream)

    def mask_bytes(self) -> ctypes.c_void_p:
        """the mask's device pointer for a reader of the bytes that works on `self.stream`: written if they were pending,
        notes kept (`mask.ptr` is for writers: it materializes too, then drops what the pipeline knew of the bytes)"""
        self._materialize_mask()
        return self.mask.raw

    # out_mask is the reference's throw-away `np.zeros_like` of styles.py:3190: the flood writes `fill` into it and the
    # caller turns it into `mask[out_mask.astype(bool)] = 254`.  The pipeline keeps it as what the flood really produces
    # -- the reached bit plane -- and writes the bytes only when somebody looks at them: `_out_pending` remembers a
    # deferred `out_mask[reached] = fill` over bytes that are known to be zero.  Zeroing it again is then free, and the
    # next flood does not have to read it.  Every path that reads or exposes the bytes calls _materialize_out() first.
    def _out_logically_zero(self) -> bool:
        return self._out_bytes_zero and self._out_pending is None

    def _materialize_out(self):
        if self._out_pending is not None:
            L.check(L.lib().ivx_dev_flood_apply(ctypes.byref(self.plan), self.reached.ptr, L.U8, self.out_mask.raw,
                                                ctypes.c_double(self._out_pending), self.stream))
            self._out_pending = None
            self._out_bytes_zero = False

    def _out_touched(self):
        self._materialize_out()
        self._out_bytes_zero = False

    def zero_out_mask(self):
        """out_mask = zeros (the np.zeros of styles.py:3190)"""
        self._materialize_mask()
        if not self._out_bytes_zero:
            L.check(L.lib().ivx_memset(self.out_mask.raw, 0, ctypes.c_size_t(self.n), self.stream))
        self._out_bytes_zero, self._out_pending = True, None

    def sync(self):
        self._materialize_mask()
        L.check(L.lib().ivx_stream_synchronize(self.stream))

    def close(self):
        if getattr(self, "stream", None) is None:
            return  # already closed (or never fully built)
        self._out_pending = None
        self._mask_pending = False
        self._prefetch = None
        if getattr(self, "flood_scratch", None) is not None and self.flood_scratch.ptr is not None:
            L.lib().ivx_dev_flood_disarm_gate(self.flood_scratch.ptr)  # an unconsumed arm must not outlive the buffers
        self._gate_armed = False
        if self._stream2 is not None:
            L.lib().ivx_stream_destroy(self._stream2)  # synchronises it first
            self._stream2 = None
        for e in self._sync_events:
            L.lib().ivx_event_destroy(e)
        self._sync_events = []
        for b in (self.image, self.mask, self.out_mask):
            b._on_touch = None  # freeing is not "somebody looked at the contents"
        self._drop_volren(all_buffers=True)
        self._drop_maskren()
        if getattr(self, "_scene3d", None) is not None:
            self._scene3d[1].close()
            self._scene3d = None
        for b in (self.image, self.mask, self.out_mask, self.cand, self.reached, self._mbits, self.flood_scratch,
                  self._mc_scratch, self._tris, self._verts, self._faces, self._gate, getattr(self, "_range_buf", None),
                  getattr(self, "_ranges", None),
                  getattr(self, "prob", None), getattr(self, "_show_tables", None), getattr(self, "_show_out", None)):
            if b is not None:
                b.close()
        self._show_tables = self._show_out = None
        if self.stream is not None:
            L.lib().ivx_stream_destroy(self.stream)
            self.stream = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def download_mask(self, out: np.ndarray | None = None) -> np.ndarray:
        self._materialize_mask()
        self.sync()
        return self.mask.download(self.shape, np.uint8, out)

    # -- edit history ---------------------------------------------------------------------------
    def snapshot_mask(self):
        """the dense mask's bytes as a `history.Snapshot` (blocks64), encoded on the volume's stream: no host byte moves"""
        from . import history

        return history.snapshot_device(self.mask_bytes(), self.n, self.shape, self.stream)

    def restore_mask(self, snapshot):
        """mask = the snapshot's state, in place on the volume's stream; what the pipeline derived from the mask's bytes
        (planes, levels, the early triangle count) is dropped as after any other mask write"""
        if snapshot.closed:
            raise ValueError("restore_mask: the snapshot has been closed")
        if snapshot.n != self.n or tuple(snapshot.shape) != self.shape:
            raise ValueError("restore_mask: the snapshot holds shape %r, the volume has %r" % (tuple(snapshot.shape), self.shape))
        self._materialize_mask()
        L.check(L.lib().ivx_dev_mask_snapshot_restore(self.mask.raw, self.n, snapshot.header.ptr, snapshot.pool.ptr,
                                                      snapshot.literal_blocks, 1, None, self.stream), "restore_mask")
        self._mask_touched()

    def download_out_mask(self) -> np.ndarray:
        self._materialize_mask()
        self._materialize_out()
        self.sync()
        return self.out_mask.download(self.shape, np.uint8)

    # -- threshold (slice_.py:1240-1247 / 1722-1769) -------------------------------------------------------
    def threshold(self, lo: int, hi: int, preserve: bool = False):
        """mask = 255 where lo <= image <= hi else 0 (with the preserve rule of do_threshold_to_a_slice when asked).
        When the rows are whole 64-voxel words the same pass also writes the mask's inside-bit plane (1/8 B/voxel
        more): it IS the candidate plane of a region growing with the same thresholds into a zero out_mask, and the
        inside plane of marching cubes at iso 127 -- both then skip their own pass over the volume.
        That pass writes the plane ONLY while a region growing is expected to follow (`_defer_pays`): the mask's bytes are
        then pending and the flood's `mask[reached] = v` writes all of them (see _materialize_mask)."""
        lib = L.lib()
        self._join_prefetch()  # a count still reading the plane must not see it change
        if self._fuse and not preserve and self.dx % 64 == 0:
            self._mbits_version += 1
            self._mp_cells_valid = False
            dims = (c64(self.dz), c64(self.dy), c64(self.dx), int(lo), int(hi))
            defer = self._mask_defer and self._defer_pays
            if self._use_ranges:
                # the first threshold of an image leaves the records behind, every later one reads them and the mixed words only
                mode = 1 if self._ranges_valid else 0  # IVX_RANGES_USE / IVX_RANGES_BUILD
                if defer:
                    L.check(lib.ivx_dev_threshold_i16_plane_ranges(self.image.raw, *dims, self._mbits.ptr, self._ranges_buffer().ptr,
                                                                   mode, self.stream), "threshold")
                else:
                    L.check(lib.ivx_dev_threshold_i16_bits_ranges(self.image.raw, *dims, self.mask.raw, self._mbits.ptr,
                                                                  self._ranges_buffer().ptr, mode, self.stream), "threshold")
                self._ranges_valid = True
            elif defer:
                L.check(lib.ivx_dev_threshold_i16_plane(self.image.raw, *dims, self._mbits.ptr, self.stream), "threshold")
            else:
                L.check(lib.ivx_dev_threshold_i16_bits(self.image.raw, *dims, self.mask.raw, self._mbits.ptr, self.stream), "threshold")
            # every byte is overwritten: an earlier pending note is dropped unwritten; with deferral this one takes its place
            self._mask_pending = defer
            self._mbits_valid, self._mbits_range = True, (int(lo), int(hi))
            self._mask_levels = (255, None)  # mask == 255 * plane, byte for byte
            return
        if preserve:
            self._materialize_mask()  # the preserve rule reads the bytes
        self._mask_pending = False
        L.check(lib.ivx_dev_threshold_i16(self.image.raw, c64(self.dz), c64(self.dy), c64(self.dx), int(lo), int(hi),
                                          int(bool(preserve)), None, self.mask.raw, self.stream), "threshold")
        self._mask_touched()

    def _ranges_buffer(self) -> DeviceBuffer:
        if self._ranges is None:
            nb = ctypes.c_size_t(0)
            L.check(L.lib().ivx_image_ranges_bytes(c64(self.dz), c64(self.dy), c64(self.dx), ctypes.byref(nb)), "image_ranges_bytes")
            self._ranges = DeviceBuffer(max(nb.value, 4))
            self._ranges_valid = False
        return self._ranges

    # -- region growing (floodfill.rs:96-166 on the image; styles.py:3151-3216) ----------------------------
    def lut_image_255(self, ww, wl) -> DeviceBuffer:
        """get_LUT_value_255(image, ww, wl) (imagedata_utils.py:540-552) as a resident int16 volume: the image the
        "dynamic" and "confidence" region-growing modes flood when use_ww_wl is set (styles.py:3166-3171, 3222-3225)."""
        self._materialize_mask()
        buf = DeviceBuffer(self.n * 2)
        L.check(L.lib().ivx_dev_lut_i16(self.image.raw, c64(self.n), ctypes.c_double(float(ww)), ctypes.c_double(float(wl)),
                                        1, buf.ptr, self.stream), "lut_image_255")
        return buf

    def region_grow(self, seeds_xyz, t0, t1, strct, fill: int = 1, select_value: int | None = 254,
                    image: DeviceBuffer | None = None) -> int:
        """floodfill_threshold(image, seeds, t0, t1, fill, strct, out_mask) followed (when select_value is not None)
        by `mask[out_mask.astype(bool)] = select_value` (styles.py:3214).  `image` = an alternative resident int16
        volume (e.g. lut_image_255).  Returns the number of global rounds."""
        lib = L.lib()
        img_ptr = image.ptr if image is not None else self.image.raw
        s3 = np.ascontiguousarray(strct, dtype=np.uint8)
        bits = ctypes.c_uint32(0)
        L.check(lib.ivx_flood_strct_bits(L.ptr(s3), L.i64(s3.shape), ctypes.byref(bits)))
        self.plan.strct_bits = bits.value
        seeds = np.ascontiguousarray(np.array([tuple(s) for s in seeds_xyz], dtype=np.int64).reshape(-1, 3))
        p = ctypes.byref(self.plan)
        st = self.stream
        t0, t1 = float(int(t0)), float(int(t1))  # wrapper int() truncation for integer images
        self._before_flood()
        cand, shared = self._candidate_plane(image, t0, t1, fill)
        rounds = ctypes.c_int(0)
        write = self._flood_write(fill, select_value) if self._select else None
        # clear + seed + run (an in-range seed is already a candidate here: the kernel's OR is a no-op on a shared plane)
        piece = self._piece_to_ride(write, shared, select_value)
        if piece is not None:
            # ... and marching cubes' count of the piece the last surface call took, in the launch of that write: nothing in the
            # step reads the mask bytes the write produces, and the count reads the inside plane only, which this write leaves
            # as it is -- the count's dependent loads run under the write's stores instead of behind them
            counted = ctypes.c_int(0)
            L.check(lib.ivx_dev_flood_grow_select_count(p, L.I16, img_ptr, ctypes.c_double(t0), ctypes.c_double(t1), L.ptr(seeds),
                                                        c64(len(seeds)), cand.ptr, self.reached.ptr, self.flood_scratch.ptr,
                                                        ctypes.byref(rounds), ctypes.byref(write), int(self._look_ahead),
                                                        ctypes.byref(piece[0]), self._mc_scratch.ptr, ctypes.byref(counted), st),
                    "region_grow")
            if counted.value:
                self._ride.rode(self._mbits_version)
            else:
                self._ride.drop()  # (the call has reset the scratch's piece record)
        elif write is not None:
            # ... and the one kernel _apply_reached would queue, from the same call: it is in the stream when Python gets back
            L.check(lib.ivx_dev_flood_grow_select(p, L.I16, img_ptr, ctypes.c_double(t0), ctypes.c_double(t1), L.ptr(seeds),
                                                  c64(len(seeds)), cand.ptr, self.reached.ptr, self.flood_scratch.ptr,
                                                  ctypes.byref(rounds), ctypes.byref(write), int(self._look_ahead), st), "region_grow")
        else:
            L.check(lib.ivx_dev_flood_grow(p, L.I16, img_ptr, ctypes.c_double(t0), ctypes.c_double(t1), L.ptr(seeds),
                                           c64(len(seeds)), cand.ptr, self.reached.ptr, self.flood_scratch.ptr,
                                           ctypes.byref(rounds), st), "region_grow")
        self._gate_armed = False  # an armed gate has been opened by this flood
        self._apply_reached(fill, select_value, shared, queued=write is not None)
        return rounds.value

    def _piece_to_ride(self, write, shared, select_value):
        """(params, z0) of the piece whose count this region growing's write can carry, or None: the write is one of the two
        from the bit planes, the inside plane is the flood's own candidate plane and stays what it is (select_value >= 127),
        the surface call before this one counted that piece from the plane into the scratch and buffer that are still there,
        no prefetch is using them, and the timer brackets neither of the two kernels (their spans keep their meaning)."""
        if (write is None or write.kind not in (L.FLOOD_WRITE_MASK_FROM_PLANES, L.FLOOD_WRITE_APPLY_LEVELS) or not shared
                or select_value is None or int(select_value) < 127 or not self._fuse or self._prefetch is not None
                or self._mc_scratch is None or self._tris is None or self.timer.records("mc_count")
                or self.timer.records("mask_bytes")):
            return None
        piece = self._ride.piece_to_ride()
        if piece is None or piece[1] != 0 or piece[0].ny != self.dy or piece[0].nx != self.dx or piece[0].nz > self.dz:
            return None
        return piece

    def flood_visits(self):
        """(tile visits, length of the first round's list) of the last flood of this volume (L.flood_visits)"""
        self._materialize_mask()
        return L.flood_visits(self.plan, self.flood_scratch.ptr, self.stream)

    def _before_flood(self):
        """the reached plane is about to be cleared: a deferred out_mask write that is still wanted must land first, and a
        note that describes the mask's bytes through that plane dies with it"""
        self._materialize_out()
        if self._mask_levels is not None and self._mask_levels[1] is not None:
            self._materialize_mask()
            self._mask_levels = None

    def _candidate_plane(self, image, t0, t1, fill):
        """The flood's candidate plane: in range AND out_mask != fill.  With out_mask known to be zero (fill != 0) and
        the mask's plane known to be "image in [t0, t1]", the plane the threshold pass left behind is exactly that and
        no pass over the volume is needed.  Returns (buffer, shared?)."""
        shared = (image is None and self._mbits_valid and self._out_logically_zero() and int(fill) != 0
                  and self._mbits_range == (int(t0), int(t1)))
        if shared:
            return self._mbits, True
        # out_mask's bytes known to be zero (fill's byte is not): nothing is barred, and reading 1 B/voxel to learn that is a
        # pass over memory for nothing
        bar, bar_mode = (None, 0) if (self._out_logically_zero() and (int(fill) & 0xff) != 0) else (self.out_mask.raw, 1)
        if image is None and self._use_ranges and self._ranges_valid:
            L.check(L.lib().ivx_dev_flood_candidates_ranges(ctypes.byref(self.plan), self.image.raw, ctypes.c_double(t0),
                                                            ctypes.c_double(t1), bar, bar_mode, ctypes.c_double(fill),
                                                            self._ranges.ptr, self.cand.ptr, self.stream), "flood_candidates_ranges")
            return self.cand, False
        img_ptr = image.ptr if image is not None else self.image.raw
        L.check(L.lib().ivx_dev_flood_candidates(ctypes.byref(self.plan), L.I16, img_ptr, ctypes.c_double(t0),
                                                 ctypes.c_double(t1), bar, bar_mode, ctypes.c_double(fill),
                                                 self.cand.ptr, self.stream))
        return self.cand, False

    def _write_kind(self, fill, select_value):
        """Which single kernel writes the flood's result while out_mask's write can be deferred (L.FLOOD_WRITE_*), from the
        volume's notes alone -- the flood's outcome has no say; None where out_mask's bytes have to be written as well."""
        if not (self._out_logically_zero() and int(fill) != 0):
            return None
        if select_value is not None and self._mask_levels == (255, None) and self._mbits_valid and self._apply_levels:
            # the mask's bytes are still to be written: one pass writes all of them, the selected ones as select_value; or
            # mask == 255 * plane, byte for byte: a touched chunk's bytes follow from the two bit planes, no byte is read
            return L.FLOOD_WRITE_MASK_FROM_PLANES if self._mask_pending else L.FLOOD_WRITE_APPLY_LEVELS
        return L.FLOOD_WRITE_APPLY_U8 if select_value is not None else L.FLOOD_WRITE_NONE

    def _flood_write(self, fill, select_value):
        """The write for ivx_dev_flood_grow_select to queue behind the flood it is about to run, or None where the two calls
        stay: out_mask's bytes are due too (ivx_dev_flood_apply2 or its own pass), or the timer wants the write's span."""
        kind = self._write_kind(fill, select_value)
        if kind is None or (kind == L.FLOOD_WRITE_MASK_FROM_PLANES and self.timer.records("mask_bytes")):
            return None
        if kind == L.FLOOD_WRITE_APPLY_U8:
            self._materialize_mask()  # that kernel changes bytes of a mask that has to be there: the flood does not touch it
        return L.FloodWrite(kind=kind, v_in=255, v_sel=int(select_value) if select_value is not None else 0,
                            inside_bits=self._mbits.ptr.value, mask=self.mask.raw.value)

    def _apply_reached(self, fill, select_value, shared, queued=False):
        """out_mask[reached] = fill and, when asked, mask[reached] = select_value; keeps the notes in step.
        `queued`: ivx_dev_flood_grow_select has queued the kernel of _write_kind() already."""
        lib, p, st = L.lib(), ctypes.byref(self.plan), self.stream
        if select_value is not None:
            self._mp_cells_valid = False
        kind = self._write_kind(fill, select_value)
        assert kind is not None or not queued
        if kind not in (L.FLOOD_WRITE_MASK_FROM_PLANES, L.FLOOD_WRITE_APPLY_LEVELS):
            self._materialize_mask()
        else:
            self._defer_pays = True  # a threshold's mask met the flood's apply untouched: the next one defers (again)
        if kind is not None:
            self._out_pending = int(fill)  # bytes stay zero; self.reached carries the result until it is needed
            if kind == L.FLOOD_WRITE_MASK_FROM_PLANES:
                if not queued:
                    with self.timer.span("mask_bytes"):
                        L.check(lib.ivx_dev_mask_from_planes(p, self._mbits.ptr, self.reached.ptr, self.mask.raw, 255,
                                                             int(select_value), st), "mask_from_planes")
                self._mask_pending = False
            elif kind == L.FLOOD_WRITE_APPLY_LEVELS and not queued:
                L.check(lib.ivx_dev_flood_apply_levels(p, self.reached.ptr, self._mbits.ptr, self.mask.raw, 255, int(select_value), st),
                        "flood_apply_levels")
            elif kind == L.FLOOD_WRITE_APPLY_U8 and not queued:
                L.check(lib.ivx_dev_flood_apply(p, self.reached.ptr, L.U8, self.mask.raw, ctypes.c_double(int(select_value)), st))
        elif select_value is not None:
            L.check(lib.ivx_dev_flood_apply2(p, self.reached.ptr, self.out_mask.raw, int(fill), self.mask.raw,
                                             int(select_value), st))
            self._out_bytes_zero = False
        else:
            L.check(lib.ivx_dev_flood_apply(p, self.reached.ptr, L.U8, self.out_mask.raw, ctypes.c_double(fill), st))
            self._out_bytes_zero = False
        if select_value is not None:
            # the mask's bytes stay known when it was 255 * plane and the selected voxels become another inside value
            lv = self._mask_levels
            self._mask_levels = (lv[0], int(select_value)) if (lv is not None and lv[1] is None and int(select_value) >= 127
                                                                and self._mbits_valid) else None
        if select_value is not None and self._mbits_valid and not (shared and int(select_value) >= 127):
            # mask[reached] = select_value: keep the inside plane in step (reached is a subset of a shared plane)
            self._join_prefetch()
            self._mbits_version += 1
            L.check(lib.ivx_dev_bits_combine(self._mbits.ptr, self.reached.ptr, c64(self._plane_words),
                                             0 if int(select_value) >= 127 else 1, st))
            self._mbits_range = None

    def region_grow_confidence(self, seed_xyz, strct, confid_mult=2.5, confid_iters=3, select_value=254,
                               image: DeviceBuffer | None = None):
        """do_rg_confidence (invesalius/data/styles.py:3220-3251): `confid_iters` rounds of
        mean +- confid_mult * std over the grown region -> floodfill_threshold into the SAME out_mask (never cleared:
        SURVEY quirk Q4).  Statistics are exact integer sums on the GPU; mean/std are formed in float64 on the host
        (std = sqrt(E[x^2] - mean^2): differs from numpy's two-pass value by rounding only, far below the int()
        truncation the wrapper applies to t0/t1)."""
        self._materialize_mask()
        lib = L.lib()
        x, y, z = (int(v) for v in seed_xyz)
        sel = np.zeros(self.shape, np.uint8)
        sel[max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 1  # styles.py:3226-3235
        d_sel = DeviceBuffer(self.n)
        d_sel.upload(sel)
        rounds = 0
        for _ in range(int(confid_iters)):
            acc = (ctypes.c_int64 * 3)()
            L.check(lib.ivx_dev_masked_stats_i16(image.ptr if image is not None else self.image.raw, d_sel.ptr, c64(self.n),
                                                 acc, self.stream))
            cnt, s1, s2 = int(acc[0]), int(acc[1]), int(acc[2])
            mean = s1 / cnt
            var = max(s2 / cnt - mean * mean, 0.0)
            std = float(np.sqrt(var))
            t0, t1 = mean - std * confid_mult, mean + std * confid_mult
            rounds += self.region_grow([(x, y, z)], t0, t1, strct, fill=1, select_value=None, image=image)
            self._materialize_out()
            L.check(lib.ivx_dev_or_equal_u8(d_sel.ptr, self.out_mask.raw, c64(self.n), 1, self.stream))
        if select_value is not None:
            self._materialize_out()
            L.check(lib.ivx_dev_flood_apply_where(self.mask.ptr, self.out_mask.raw, c64(self.n), 1, int(select_value),
                                                  self.stream))  # mask.ptr: drops the inside-plane note
        self.sync()
        d_sel.close()
        return rounds

    # -- slice editing tools ---------------------------------------------------------------
    def _slice_geometry(self, orientation: str, n: int):
        """(h, w, first element, row stride, element stride) of slice `n` in a dense (dz, dy, dx) block, in elements"""
        ax = {"AXIAL": 0, "CORONAL": 1, "SAGITAL": 2}.get(orientation)
        if ax is None:
            raise ValueError("orientation must be AXIAL, CORONAL or SAGITAL")
        if not 0 <= int(n) < self.shape[ax]:
            raise IndexError("slice %d outside the volume" % n)
        st = (self.dy * self.dx, self.dx, 1)
        r, e = (a for a in range(3) if a != ax)
        return self.shape[r], self.shape[e], int(n) * st[ax], st[r], st[e]

    def brush_stroke(self, orientation: str, n: int, index, positions, operations=2, edition_threshold_range=(0, 0),
                     fill_value: int = 0, target: DeviceBuffer | None = None):
        """slice_.edit_mask_stroke on the resident mask (or on `target`, a uint8 block of the volume's shape, e.g. watershed
        markers): the dabs of `positions` under the footprint `index` on slice `n`, in maximal runs of one operation launched
        in order on the volume's stream (ivx_dev_mask_brush_stroke).  The resident mask has no flag cells."""
        from . import cursor
        from . import slice_ as sl

        h, w, first, rs, es = self._slice_geometry(orientation, n)
        if np.ndim(index) != 2:
            raise TypeError("the footprint is a 2-D array")
        fp = np.ascontiguousarray(np.asarray(index) != 0).view(np.uint8)
        positions = list(positions)
        runs = sl._op_runs(operations, len(positions))
        if not runs or fp.size == 0:
            return
        dabs = cursor.dab_windows(positions, fp.shape, w)
        lo, hi = sl._int_bounds(edition_threshold_range)
        base = (target.ptr if target is not None else self.mask.ptr).value  # (mask.ptr: a writer's pointer, the notes drop)
        d_fp, d_dabs = DeviceBuffer(fp.size), DeviceBuffer(dabs.nbytes)
        try:
            d_fp.upload(fp)
            d_dabs.upload(dabs)
            at = 0
            for op, k in runs:
                L.check(L.lib().ivx_dev_mask_brush_stroke(
                    ctypes.c_void_p(base + first), c64(rs), c64(es), ctypes.c_void_p(self.image.raw.value + first * 2), c64(rs * 2),
                    c64(es * 2), c64(h), c64(w), d_fp.ptr, c64(fp.shape[0]), c64(fp.shape[1]), d_dabs.at(at * 8), c64(k), int(op),
                    int(lo), int(hi), int(fill_value) & 255, self.stream), "brush_stroke")
                at += k
            L.check(L.lib().ivx_stream_synchronize(self.stream))
        finally:
            d_fp.close()
            d_dabs.close()

    def brush_fill(self, orientation: str, n: int, fill_value: int, index, positions, target: DeviceBuffer | None = None):
        """styles.brush_fill on a resident block: `fill_value` under the footprint at every position"""
        self.brush_stroke(orientation, n, index, positions, 6, fill_value=fill_value, target=target)

    def crop_mask(self, limits):
        """styles.crop_mask on the resident mask -- the interior ``matrix[1:, 1:, 1:]`` -- so the kept box
        ``[zi : zf + 2, ...]`` of the padded matrix is ``[zi - 1 : zf + 1, ...]`` here; everything else becomes 1."""
        xi, xf, yi, yf, zi, zf = (int(v) for v in limits)
        if min(xi, yi, zi) < 0 or min(xf, yf, zf) < -2:
            raise ValueError("crop limits must not be negative")
        box = L.i64([max(zi - 1, 0), min(zf + 1, self.dz), max(yi - 1, 0), min(yf + 1, self.dy), max(xi - 1, 0), min(xf + 1, self.dx)])
        L.check(L.lib().ivx_dev_mask_crop(self.mask.ptr, c64(self.dz), c64(self.dy), c64(self.dx), box, self.stream), "crop_mask")

    # -- the 3-D mask editor ---------------------------------------------------------------
    def _m3e_flags(self) -> DeviceBuffer:
        f = getattr(self, "_m3e_plane_flags", None)
        if f is None or f.nbytes < self.dz:
            if f is not None:
                f.close()
            f = self._m3e_plane_flags = DeviceBuffer(self.dz)
        f.zero(self.stream)
        return f

    def _m3e_geometry(self):
        return L.i64(self.shape), L.i64((self.dy * self.dx, self.dx, 1))  # the voxels alone: no flag planes

    def cut_mask(self, polygons, size, m, mv, depth, edit_mode) -> np.ndarray:
        """mask3d_editor.cut_mask on the resident mask, on the volume's stream: the screen filter of the `polygons` (display
        points) for the viewport `size` = (w, h), then mask_cut with the matrices `m` / `mv` down to the distance `depth`.
        Returns one flag per axial slice that changed.  Planes, levels and the early triangle count go, as after any write."""
        from . import mask3d_editor as M3

        w, h = int(size[0]), int(size[1])
        mode = M3._filter_mode(edit_mode)
        points, offsets = M3._pack_polygons(polygons)
        m, mv = M3._mat4(m, "m"), M3._mat4(mv, "mv")
        lib = L.lib()
        blk = DeviceBuffer(points.nbytes + offsets.nbytes + 16 + h * w)
        try:
            blk.upload(np.concatenate([offsets.view(np.uint8), points.reshape(-1).view(np.uint8)]))
            d_f = blk.at(offsets.nbytes + points.nbytes)
            L.check(lib.ivx_dev_m3e_filter(w, h, blk.at(offsets.nbytes), blk.at(0), len(offsets) - 1, mode, d_f, self.stream), "cut_mask")
            shape, strides = self._m3e_geometry()
            flags = self._m3e_flags()
            L.check(lib.ivx_dev_m3e_cut(self.mask.ptr, shape, strides, M3._d3(self.spacing), float(depth), d_f, h, w, L.ptr(m), L.ptr(mv),
                                        mode, flags.ptr, self.stream), "cut_mask")
            L.check(lib.ivx_stream_synchronize(self.stream))
            return flags.download((self.dz,), np.uint8).astype(bool)
        finally:
            blk.close()

    def brush_mask_stroke(self, world_coords, brush_size, edit_mode, orig: DeviceBuffer | None = None) -> np.ndarray:
        """mask3d_editor.brush_stroke on the resident mask, on the volume's stream: one dab per world point, the whole drag in
        one launch per `mask3d_editor.brush_capacity()` dabs.  `orig`: a uint8 block of the volume's shape that include mode
        reveals (None: 255 is painted).  Returns one flag per axial slice that changed."""
        from . import mask3d_editor as M3

        centres = M3.brush_centres(world_coords, self.spacing)
        d_c = DeviceBuffer(max(centres.nbytes, 16))
        try:
            d_c.upload(centres)
            shape, strides = self._m3e_geometry()
            flags = self._m3e_flags()
            L.check(L.lib().ivx_dev_m3e_brush_stroke(self.mask.ptr, orig.ptr if orig is not None else None, shape, strides,
                                                     M3._d3(self.spacing), L.ptr(centres), d_c.ptr, len(centres), float(brush_size) / 2.0,
                                                     int(edit_mode), flags.ptr, self.stream), "brush_mask_stroke")
            L.check(L.lib().ivx_stream_synchronize(self.stream))
            return flags.download((self.dz,), np.uint8).astype(bool)
        finally:
            d_c.close()

    # -- slice display ---------------------------------------------------------------------
    def _image_min_max(self):
        """(min, max) of the resident image as int16 numbers, as ``Slice.matrix.min()`` gives them; kept while `image_range()`
        holds"""
        if not self._range_valid or getattr(self, "_range_host", None) is None:
            buf = self.image_range()
            L.check(L.lib().ivx_stream_synchronize(self.stream))
            lo, hi = buf.download((2,), np.float32)
            self._range_host = (np.int16(lo), np.int16(hi))
        return self._range_host

    def show_slice(self, orientation: str, n: int, state, image: DeviceBuffer | None = None, image_dtype=np.int16, mask: bool = True,
                   aux: DeviceBuffer | None = None, image_range=None, download: bool = True):
        """slice_.get_slices on the resident volume: the (h, w, 3) uint8 picture of slice `n` from one launch of
        ivx_dev_slice_show on the volume's stream, reading the image, the resident mask and `aux` in place through their
        strides (a sagittal slice is gathered by the kernel).  `image`: the dense (h, w) device output of a projection kernel
        (`project`, `mida`, the resampler; `image_dtype` int16, or float64 for MeanIP) shown in place of the plain slice.
        `mask`: there is a current mask (the resident one, drawn when ``state.mask_shown``; it has no flag cells, so no lazy
        threshold).  `aux`: the uint8 block of the volume's shape that ``state.to_show_aux`` names (`self.mask` for SELECT).
        Returns the picture, or with ``download=False`` the DeviceBuffer that holds it (valid until the next call, queued on
        `self.stream`)."""
        from . import slice_display as D

        h, w, first, rs, es = self._slice_geometry(orientation, n)
        kind = {np.dtype(np.int16): D.IMG_I16, np.dtype(np.float64): D.IMG_F64}.get(np.dtype(image_dtype))
        if kind is None:
            raise TypeError("image_dtype must be int16 or float64")
        isz = 2 if kind == D.IMG_I16 else 8
        if image is not None:
            if image.nbytes < h * w * isz:
                raise ValueError("the projection's block holds %d bytes, the picture needs %d" % (image.nbytes, h * w * isz))
            ip, irs, ies = image.ptr, w * isz, isz
        else:
            if kind != D.IMG_I16:
                raise TypeError("the resident image is int16")
            ip, irs, ies = self.image.raw_at(first * 2), rs * 2, es * 2
        mp = None
        if mask and state.mask_shown:
            mp = ctypes.c_void_p(self.mask_bytes().value + first)
        aux_colours = D.aux_colour_dict(state, bool(mask))
        ap = None
        if aux_colours is not None:
            if aux is None:
                raise TypeError("the aux overlay %r needs its device block" % state.to_show_aux)
            if aux.nbytes < self.n:
                raise ValueError("the aux block is smaller than the volume")
            base = self.mask_bytes() if aux is self.mask else aux.ptr
            ap = ctypes.c_void_p(base.value + first)
        if state.from_ == D.OTHER and image_range is None:
            image_range = self._image_min_max()
        p, blob = D.build(state, kind, D.ST_ALL, image_range=image_range, have_mask=mp is not None, aux_colours=aux_colours)
        if getattr(self, "_show_tables", None) is None or self._show_tables.nbytes < blob.nbytes:
            self._show_tables = DeviceBuffer(3072 + 32 * D.MAX_NODES)
        if getattr(self, "_show_out", None) is None or self._show_out.nbytes < h * w * 3:
            self._show_out = DeviceBuffer(h * w * 3)
        L.check(L.lib().ivx_stream_synchronize(self.stream))  # (an earlier picture's launch may still read the tables block)
        self._show_tables.upload(blob)
        L.check(L.lib().ivx_dev_slice_show(ip, c64(irs), c64(ies), mp, c64(rs), c64(es), ap, c64(rs), c64(es), c64(h), c64(w), ctypes.byref(p),
                                           self._show_tables.ptr, self._show_out.ptr, self.stream), "show_slice")
        if not download:
            return self._show_out
        L.check(L.lib().ivx_stream_synchronize(self.stream))
        return self._show_out.download((h, w, 3), np.uint8)

    # -- density measures ---------------------------------------------------------------------
    def roi_records(self, measures, spacing=None) -> np.ndarray:
        """the (R, 5) int64 records cnt, s1, s2, lo, hi of `measures` (measures.CircleDensityMeasure / PolygonDensityMeasure) on
        the resident image: one memset and one launch of ivx_dev_roi_density on the volume's stream, reading the slices in
        place through their strides; descriptors and points go up, 40 bytes per measure come down"""
        from . import measures as M

        grid = M._Grid(self.image.raw_at(0).value, self.shape, (self.dy * self.dx * 2, self.dx * 2, 2))
        q, points = M.describe_rois(grid, self.spacing if spacing is None else spacing, measures)
        n = len(measures)
        out = np.zeros((n, 5), np.int64)
        if not n:
            return out
        if getattr(self, "_roi_records", None) is None or self._roi_records.nbytes < n * L.ROI_RECORD_BYTES:
            self._roi_records = DeviceBuffer(max(n, 64) * L.ROI_RECORD_BYTES)
        pp = None
        if len(points):
            if getattr(self, "_roi_points", None) is None or self._roi_points.nbytes < points.nbytes:
                self._roi_points = DeviceBuffer(max(points.nbytes, 4096))
            L.check(L.lib().ivx_stream_synchronize(self.stream))  # (an earlier batch's launch may still read the points block)
            self._roi_points.upload(points)
            pp = self._roi_points.ptr
        L.check(L.lib().ivx_dev_roi_density(q, c64(n), L.ptr(points) if len(points) else None, pp, c64(len(points)), self._roi_records.ptr,
                                            self.stream), "roi_density")
        L.check(L.lib().ivx_stream_synchronize(self.stream))
        return self._roi_records.download((n, 5), np.int64, out)

    def roi_density(self, rois):
        """`measures.density_of` on the resident image: a list of density measures or ``measurements.plist`` dicts in, their
        results out, no host array involved"""
        from . import measures as M

        return M.density_of(self, self.spacing, rois)

    # -- image geometry tools ----------------------------------------------------------------
    def _after_image_geometry(self, shape=None, spacing=None):
        """The image's voxels moved (flip, swap axes, gantry tilt): everything derived from the image goes, as in
        `_image_touched` -- min/max records, cached range, volume-render field -- and so does everything derived from the
        mask, which the reference clears (slice_.py:2136-2146): the mask and the out mask become zeros, the notes about their
        bytes, the mask-render cells, the flood's planes and its gate are dropped.  A new `shape` rebuilds what is sized by it."""
        lib = L.lib()
        self._mask_pending = False   # the deferred bytes are about to be zeros anyway
        self._out_pending = None
        self._image_touched()
        self._drop_maskren()
        self._mbits_valid, self._mbits_range, self._mask_levels = False, None, None
        self._mbits_version += 1
        self._mc_params_cache = {}
        if self._gate_armed:
            L.check(lib.ivx_dev_flood_disarm_gate(self.flood_scratch.ptr))
            self._gate_armed = False
        if spacing is not None:
            self.spacing = tuple(float(s) for s in spacing)
        if shape is not None and tuple(shape) != self.shape:
            self.sync()
            self.shape = tuple(int(s) for s in shape)
            self.dz, self.dy, self.dx = self.shape
            for name in ("cand", "reached", "_mbits", "flood_scratch", "_mc_scratch", "_tris", "_verts", "_faces", "_ranges", "_range_buf"):
                b = getattr(self, name, None)
                if b is not None:
                    b.close()
                setattr(self, name, None)
            self._ranges_valid = self._range_valid = False
            self.plan = L.FloodPlan(self.dz, self.dy, self.dx, (self.dx + 63) // 64, 0)
            nb, ns = ctypes.c_size_t(0), ctypes.c_size_t(0)
            L.check(lib.ivx_flood_bits_bytes(ctypes.byref(self.plan), ctypes.byref(nb)))
            L.check(lib.ivx_flood_scratch_bytes(ctypes.byref(self.plan), ctypes.byref(ns)))
            self.cand, self.reached, self._mbits = DeviceBuffer(nb.value), DeviceBuffer(nb.value), DeviceBuffer(nb.value)
            self._plane_words = nb.value // 8
            self.flood_scratch = DeviceBuffer(ns.value)
        L.check(lib.ivx_memset(self.mask.raw, 0, ctypes.c_size_t(self.n), self.stream))
        L.check(lib.ivx_memset(self.out_mask.raw, 0, ctypes.c_size_t(self.n), self.stream))
        self._out_bytes_zero = True

    def flip(self, axis: int):
        """slice_.flip_volume on the resident image (Slice.OnFlipVolume, slice_.py:2103-2149): in place in HBM; the mask is
        cleared and everything derived from image or mask is dropped."""
        if axis not in (0, 1, 2):
            raise ValueError("axis must be 0, 1 or 2")
        self._join_prefetch()
        L.check(L.lib().ivx_dev_image_flip(self.image.raw, c64(self.dz), c64(self.dy), c64(self.dx), 2, int(axis), self.stream), "flip")
        self._after_image_geometry()

    def swap_axes(self, axes):
        """slice_.swap_volume_axes on the resident image (Slice.OnSwapVolumeAxes, slice_.py:2151-2251): the image becomes
        ``np.array(image.swapaxes(*axes))`` through a second block in HBM, shape and spacing follow, the mask is cleared."""
        from .slice_ import swapped_spacing

        a, b = (int(v) for v in axes)
        if a == b or not {a, b} <= {0, 1, 2}:
            raise ValueError("axes must be two different ones of 0, 1, 2")
        self._join_prefetch()
        out = DeviceBuffer(self.n * 2)
        try:
            L.check(L.lib().ivx_dev_image_swap_axes(self.image.raw, c64(self.dz), c64(self.dy), c64(self.dx), 2, a, b, out.ptr, self.stream),
                    "swap_axes")
            L.check(L.lib().ivx_memcpy_d2d(self.image.raw, out.ptr, ctypes.c_size_t(self.n * 2), self.stream), "swap_axes copy")
            L.check(L.lib().ivx_stream_synchronize(self.stream))  # the block goes out of scope here
        finally:
            out.close()
        shape = list(self.shape)
        shape[a], shape[b] = shape[b], shape[a]
        self._after_image_geometry(shape, swapped_spacing(self.spacing, (a, b)))

    def fix_gantry_tilt(self, tilt, scratch_bytes: int | None = None):
        """slice_.fix_gantry_tilt on the resident image (imagedata_utils.FixGantryTilt, imagedata_utils.py:143-154), with the
        volume's own spacing; `scratch_bytes` bounds the coefficient slab (the result does not depend on it).  Returns the
        fill value of every slice."""
        from .slice_ import gantry_tilt_shifts

        shifts = gantry_tilt_shifts(self.dz, self.spacing, tilt)
        cvals = np.zeros(self.dz, np.int32)
        if self.n == 0:
            return cvals
        nb = ctypes.c_size_t(0)
        L.check(L.lib().ivx_image_tilt_scratch_bytes(c64(self.dz), c64(self.dy), c64(self.dx), ctypes.byref(nb)), "tilt_scratch_bytes")
        self._join_prefetch()
        scratch = DeviceBuffer(nb.value if scratch_bytes is None else int(scratch_bytes))
        try:
            L.check(L.lib().ivx_dev_image_fix_gantry_tilt(self.image.raw, c64(self.dz), c64(self.dy), c64(self.dx), L.ptr(shifts),
                                                          scratch.ptr, ctypes.c_size_t(scratch.nbytes), L.ptr(cvals), self.stream),
                    "fix_gantry_tilt")
            L.check(L.lib().ivx_stream_synchronize(self.stream))  # the scratch goes out of scope here
        finally:
            scratch.close()
        self._after_image_geometry()
        return cvals

    def reached_count(self) -> int:
        self._materialize_mask()
        n = ctypes.c_int64(0)
        L.check(L.lib().ivx_dev_flood_count(ctypes.byref(self.plan), self.reached.ptr, ctypes.byref(n), self.stream))
        return n.value

    # -- marching cubes over the whole resident volume (surface_process.py:100-186) ------------------------
    def _mc_params(self, from_binary, min_value, max_value, fill_border_holes=True, z0=0, z1=None, roi_start=None,
                   pad_bottom=None, pad_top=None) -> L.McParams:
        z1 = self.dz if z1 is None else z1
        key = (bool(from_binary), min_value, max_value, bool(fill_border_holes), z0, z1, roi_start, pad_bottom, pad_top,
               tuple(self.spacing))
        hit = self._mc_params_cache.get(key)
        if hit is not None:
            return hit
        p = L.McParams()
        pb = (z0 == 0) if pad_bottom is None else pad_bottom
        pt = (z1 >= self.dz) if pad_top is None else pad_top
        if fill_border_holes:
            p.pad_xy, p.pad_bottom, p.pad_top, p.vtk_pz = 1, int(pb), int(pt), int(pb)
        else:
            p.pad_xy = p.pad_bottom = p.pad_top = p.vtk_pz = 0
        p.nz, p.ny, p.nx = z1 - z0, self.dy, self.dx
        p.roi_start = z0 if roi_start is None else roi_start
        p.spacing[:] = self.spacing
        if from_binary:
            p.dtype, p.niso, p.pad_value = L.U8, 1, 0.0
            p.iso[:] = [127.0, 0.0]
        else:
            p.dtype, p.niso, p.pad_value = L.I16, 2, float(np.iinfo(np.int16).min)
            p.iso[:] = [float(min_value), float(max_value)]
        if len(self._mc_params_cache) < 64:
            self._mc_params_cache[key] = p  # callers treat the struct as read-only
        return p

    # -- marching cubes -----------------------------------------------------------------------------------------------
    def _surface_params(self, from_binary, min_value, max_value, fill_border_holes):
        """(piece parameters, first slice) of this volume's surface call; SlabVolume answers with its slab's piece"""
        return self._mc_params(from_binary, min_value, max_value, fill_border_holes), 0

    def _mc_setup(self, p, z0):
        """scratch of the right size, the voxel source and -- when the pipeline still holds it -- the inside plane"""
        nb = ctypes.c_size_t(0)
        L.check(L.lib().ivx_dev_mc_scratch_bytes(ctypes.byref(p), ctypes.byref(nb)))
        if self._mc_scratch is None or self._mc_scratch.nbytes < nb.value:
            self._join_prefetch()
            self._ride.drop()
            if self._mc_scratch is not None:
                self.sync()  # (marching_cubes returns with the emit still queued: it reads the block about to be freed)
                self._mc_scratch.close()
            self._mc_scratch = DeviceBuffer(nb.value)
        isz = 1 if p.dtype == L.U8 else 2
        src = (self.mask if p.dtype == L.U8 else self.image).raw_at(z0 * self.dy * self.dx * isz)
        plane = None
        if (p.dtype == L.U8 and p.niso == 1 and p.iso[0] == 127.0 and self._mbits_valid and p.ny == self.dy
                and p.nx == self.dx):
            plane = self._mbits.at(z0 * self.dy * ((self.dx + 63) // 64) * 8)
        return src, plane

    def _levels(self, p, plane, z0):
        """The known byte levels of the mask as `_MaskLevels`, when the pipeline can prove them -- 0 outside the inside plane
        `plane`, `v_in` inside it and `v_sel` where the plane `sel` has a bit --; None when it cannot: the voxels are read then.
        (A caller's own `params` may carry another padding value, or levels that do not straddle iso 127 the way the kernels'
        constants assume.)"""
        lv = self._mask_levels
        if not (plane is not None and lv is not None and self._fuse and os.environ.get("IVX_MC_LEVELS", "1") != "0"
                and float(p.pad_value) == 0.0 and lv[0] > 127 and (lv[1] is None or lv[1] > 127)):
            return None
        if lv[1] is None:
            return _MaskLevels(float(lv[0]), None, float(lv[0]))
        return _MaskLevels(float(lv[0]), self.reached.at(z0 * self.dy * ((self.dx + 63) // 64) * 8), float(lv[1]))

    def _emit(self, p, src, plane, z0, cap, stream):
        """the triangle emit of a counted piece: from the known byte levels of the mask when the pipeline can prove them
        (no voxel is read), else from the voxels"""
        lib, levels = L.lib(), self._levels(p, plane, z0)
        if levels is not None:
            # (the emit wants a plane in any case: without a second level any will do, both values are the same)
            sel = levels.sel if levels.has_second else plane
            L.check(lib.ivx_dev_mc_emit_levels(ctypes.byref(p), self._mc_scratch.ptr, sel, ctypes.c_double(0.0),
                                               ctypes.c_double(levels.v_in), ctypes.c_double(levels.v_sel), self._tris.ptr, c64(cap),
                                               stream), "mc_emit")
        else:
            L.check(lib.ivx_dev_mc_emit(ctypes.byref(p), src, self._mc_scratch.ptr, self._tris.ptr, c64(cap), stream), "mc_emit")

    def _second_stream(self):
        if self._stream2 is None:
            s = ctypes.c_void_p()
            if os.environ.get("IVX_PREFETCH_PRIORITY", "low") == "low":
                L.check(L.lib().ivx_stream_create_low_priority(ctypes.byref(s)))  # fills idle CUs, yields to the flood
            else:
                L.check(L.lib().ivx_stream_create(ctypes.byref(s)))
            self._stream2 = s
            for _ in range(2):
                e = ctypes.c_void_p()
                L.check(L.lib().ivx_event_create_sync(ctypes.byref(e)))
                self._sync_events.append(e)
        return self._stream2

    def _join_prefetch(self):
        """an outstanding prefetch is about to lose its inputs (or its scratch): let it finish, then forget it"""
        if self._prefetch is not None:
            if self._gate_armed:
                L.check(L.lib().ivx_dev_gate_open(self._gate.ptr, ctypes.c_uint32(self._gate_epoch), self.stream))
                L.check(L.lib().ivx_dev_flood_disarm_gate(self.flood_scratch.ptr))
                self._gate_armed = False
            L.check(L.lib().ivx_stream_synchronize(self._stream2))
            self._prefetch = None

    def surface_prefetch(self, from_binary=True, min_value=0, max_value=0, fill_border_holes=True,
                         behind_flood: bool = True) -> bool:
        """Queue the part of the coming `marching_cubes(...)` call (same arguments) that depends on the mask's inside
        plane only -- count, scan and triangle list -- on a second stream, NOW: it then runs under whatever follows on
        the main stream (typically the region growing, whose `mask[reached] = 254` changes values the emit
        interpolates but not which side of iso 127 a voxel is on).  Needs the plane the threshold pass left behind
        and a triangle buffer from an earlier call (its size is the capacity); returns False, doing nothing, otherwise.
        Any change to the plane in between simply voids the prefetch.  `behind_flood`: hold the prefetched passes back
        until the next region growing has left its throughput-bound first rounds (they would slow each other down;
        its latency-bound tail leaves most of the GPU idle) -- or for 300 us at most, if no region growing follows."""
        if not from_binary or not self._fuse or self._tris is None or not self._mbits_valid:
            return False
        self._join_prefetch()
        p, z0 = self._surface_params(from_binary, min_value, max_value, fill_border_holes)
        src, plane = self._mc_setup(p, z0)
        if plane is None:
            return False
        self._ride.drop()  # the prefetch counts into the same scratch
        lib, s2 = L.lib(), self._second_stream()
        cap = self._tris.nbytes // 36
        L.check(lib.ivx_event_record(self._sync_events[0], self.stream))   # the plane is complete at this point
        L.check(lib.ivx_stream_wait_event(s2, self._sync_events[0]))
        if behind_flood:
            if self._gate is None:
                self._gate = DeviceBuffer(64)
                self._gate.zero(self.stream)
                self.sync()
            self._gate_epoch = (self._gate_epoch % 0x7fffffff) + 1
            L.check(lib.ivx_dev_flood_arm_gate(self.flood_scratch.ptr, self._gate.ptr, ctypes.c_uint32(self._gate_epoch),
                                               ctypes.c_uint32(512)))
            L.check(lib.ivx_dev_gate_wait(self._gate.ptr, ctypes.c_uint32(self._gate_epoch), ctypes.c_uint32(300), s2))
            self._gate_armed = True
        L.check(lib.ivx_dev_mc_count_bits_async(ctypes.byref(p), plane, self._mc_scratch.ptr, s2), "mc_count")
        L.check(lib.ivx_dev_mc_list(ctypes.byref(p), self._mc_scratch.ptr, c64(cap), s2), "mc_list")
        self._prefetch = (p, z0, cap, self._mbits_version)
        return True

    def marching_cubes(self, from_binary=True, min_value=0, max_value=0, fill_border_holes=True, download=False,
                       params: L.McParams | None = None, z0: int = 0, out: np.ndarray | None = None):
        """count + emit on the resident mask (from_binary, iso 127) or image (two iso-values).  Returns the triangle
        count, or the (T,3,3) float32 soup when download=True (written into `out` -- e.g. a `_lib.pinned_empty` array with
        room for it -- when given).
        With download=False the count may come back while the triangle list and the emit are still queued or running: the
        soup in `self._tris` is complete in stream order.  Whatever is queued on `self.stream` afterwards (the next threshold,
        another surface) is ordered behind it by the stream; call sync() before reading the buffer from anywhere else."""
        self._materialize_mask()
        lib = L.lib()
        if params is not None:
            p = params
        else:
            p, z0 = self._surface_params(from_binary, min_value, max_value, fill_border_holes)
        pf, n = self._prefetch, ctypes.c_int64(0)
        if pf is not None:
            ok = (pf[0] is p and pf[1] == z0 and self._tris is not None and pf[2] == self._tris.nbytes // 36
                  and pf[3] == self._mbits_version and self._mbits_valid)
            if not ok:
                self._join_prefetch()
            else:
                # count and list are done or running on the second stream; the emit needs the mask's final bytes
                src, plane = self._mc_setup(p, z0)
                s2, cap = self._stream2, pf[2]
                if self._gate_armed:  # no flood came in between: open the gate by hand instead of waiting it out
                    L.check(lib.ivx_dev_gate_open(self._gate.ptr, ctypes.c_uint32(self._gate_epoch), self.stream))
                    L.check(lib.ivx_dev_flood_disarm_gate(self.flood_scratch.ptr))
                    self._gate_armed = False
                L.check(lib.ivx_event_record(self._sync_events[1], self.stream))
                L.check(lib.ivx_stream_wait_event(s2, self._sync_events[1]))
                L.check(lib.ivx_dev_mc_emit(ctypes.byref(p), src, self._mc_scratch.ptr, self._tris.ptr, c64(cap), s2), "mc_emit")
                L.check(lib.ivx_dev_mc_total(ctypes.byref(p), self._mc_scratch.ptr, ctypes.byref(n), s2), "mc_total")
                self._prefetch = None  # the host has seen the total: everything on the second stream has finished
                nt = n.value
                if nt <= cap:
                    if download:
                        return self._tris.download((nt, 3, 3), np.float32, out if out is not None and out.nbytes >= nt * 36 else None)
                    return nt
                # the surface outgrew the buffer: take the ordinary path below (it re-counts and re-emits)
        src, plane = self._mc_setup(p, z0)
        n = ctypes.c_int64(0)
        # the region growing before this call may have counted this very piece in its write's launch (mc_ride.py); a timer that
        # brackets the count gets a count to bracket
        if plane is not None and self._tris is not None and not self.timer.records("mc_count"):
            rode = self._ride.take(p, z0, self._mbits_version)
        else:
            rode = False
            self._ride.drop()
        # (armed by the first call too: it ends with a triangle buffer, which is what the steady state needs)
        self._ride.surface_counted(p, z0, plane is not None)
        if self._tris is not None:
            # steady state: the triangle buffer of the previous call gives a capacity, so count, list and emit are queued
            # back to back and the count is read afterwards (no host round trip between the two halves)
            cap = self._tris.nbytes // 36
            if not rode:
                with self.timer.span("mc_count"):
                    if plane is not None:
                        L.check(lib.ivx_dev_mc_count_bits_async(ctypes.byref(p), plane, self._mc_scratch.ptr, self.stream), "mc_count")
                    else:
                        L.check(lib.ivx_dev_mc_count_async(ctypes.byref(p), src, self._mc_scratch.ptr, self.stream), "mc_count")
            with self.timer.span("mc_emit"):
                self._emit(p, src, plane, z0, cap, self.stream)
            # the scan published the count itself: it is here long before the emit ends, and the next call's kernels can be
            # queued behind an emit that is still running
            L.check(lib.ivx_dev_mc_total_early(ctypes.byref(p), self._mc_scratch.ptr, ctypes.byref(n), self.stream), "mc_total")
            nt = n.value
            if nt > cap:  # the surface outgrew the buffer: emit again into a larger one
                self.sync()  # (the first emit may still be writing the buffer that is about to be freed)
                self._tris.close()
                self._tris = DeviceBuffer(int(nt * 36 * 1.25) + 4096)
                self._emit(p, src, plane, z0, nt, self.stream)
        else:
            with self.timer.span("mc_count"):
                if plane is not None:
                    L.check(lib.ivx_dev_mc_count_bits(ctypes.byref(p), plane, self._mc_scratch.ptr, ctypes.byref(n), self.stream),
                            "mc_count")
                else:
                    L.check(lib.ivx_dev_mc_count(ctypes.byref(p), src, self._mc_scratch.ptr, ctypes.byref(n), self.stream), "mc_count")
            nt = n.value
            self._tris = DeviceBuffer(int(nt * 36 * 1.25) + 4096)
            with self.timer.span("mc_emit"):
                self._emit(p, src, plane, z0, nt, self.stream)
        if download:
            self.sync()
            return self._tris.download((nt, 3, 3), np.float32, out if out is not None and out.nbytes >= nt * 36 else None)
        return nt

    def marching_cubes_indexed(self, from_binary=True, min_value=0, max_value=0, fill_border_holes=True, download=False,
                               params: L.McParams | None = None, z0: int = 0):
        """Same surface with coincident points merged (ivx.h "indexed surface").  Returns (n_verts, n_tris), or the
        (V,3) float32 / (T,3) int32 arrays when download=True; the device buffers stay in self._verts / self._faces."""
        self._materialize_mask()
        lib = L.lib()
        if params is not None:
            p = params
        else:
            p, z0 = self._surface_params(from_binary, min_value, max_value, fill_border_holes)
        self._join_prefetch()  # same scratch
        self._ride.drop()
        self._ride.surface_counted(p, z0, False)
        src, plane = self._mc_setup(p, z0)
        nt, nv = ctypes.c_int64(0), ctypes.c_int64(0)
        with self.timer.span("mc_count"):
            if plane is not None:
                L.check(lib.ivx_dev_mc_count_bits(ctypes.byref(p), plane, self._mc_scratch.ptr, ctypes.byref(nt), self.stream),
                        "mc_count")
            else:
                L.check(lib.ivx_dev_mc_count(ctypes.byref(p), src, self._mc_scratch.ptr, ctypes.byref(nt), self.stream), "mc_count")
        # the mask's bytes known through the pipeline's planes: neither the strictly-inside plane nor a vertex needs a voxel
        levels = self._levels(p, plane, z0)
        with self.timer.span("mci_count"):
            if levels is not None:
                L.check(lib.ivx_dev_mc_indexed_count_levels(ctypes.byref(p), self._mc_scratch.ptr, ctypes.byref(nv), self.stream),
                        "mc_indexed_count")
            else:
                L.check(lib.ivx_dev_mc_indexed_count(ctypes.byref(p), src, self._mc_scratch.ptr, ctypes.byref(nv), self.stream),
                        "mc_indexed_count")
        for name, need in (("_verts", nv.value * 12), ("_faces", nt.value * 12)):
            buf = getattr(self, name)
            if buf is None or buf.nbytes < need:
                if buf is not None:
                    buf.close()
                setattr(self, name, DeviceBuffer(int(need * 1.25) + 4096))
        with self.timer.span("mci_emit"):
            if levels is not None:
                L.check(lib.ivx_dev_mc_indexed_emit_levels(ctypes.byref(p), self._mc_scratch.ptr, levels.sel, ctypes.c_double(0.0),
                                                           ctypes.c_double(levels.v_in), ctypes.c_double(levels.v_sel), self._verts.ptr,
                                                           c64(nv.value), self._faces.ptr, c64(nt.value), self.stream),
                        "mc_indexed_emit")
            else:
                L.check(lib.ivx_dev_mc_indexed_emit(ctypes.byref(p), src, self._mc_scratch.ptr, self._verts.ptr, c64(nv.value),
                                                    self._faces.ptr, c64(nt.value), self.stream), "mc_indexed_emit")
        if download:
            self.sync()
            return self._verts.download((nv.value, 3), np.float32), self._faces.download((nt.value, 3), np.int32)
        return nv.value, nt.value

    # -- watershed (watershed_process.py:19-60 + the merge of styles.py:2147-2152) on the resident volume -------------------
    def watershed(self, markers: np.ndarray, strct, use_ww_wl: bool = False, wl=0, ww=0, overwrite: bool = False,
                  algorithm: str = "Watershed IFT", mg_size=(3, 3, 3)):
        """do_watershed followed by the caller's merge rule, all in HBM: cost image (LUT or ``image - image.min()``) ->
        [`algorithm == "Watershed"`: morphological gradient of `mg_size`] -> marker flood (`ivx_dev_watershed_ift`, or
        `ivx_dev_watershed_sk` for "Watershed", the GUI's default) -> ``mask`` gets 253 where the flood says 1 and 2 where
        it says 2 (only over cells that hold 0 / 2 / 253, or over everything after zeroing with `overwrite`).
        `markers`: int8 / int16 (0, 1, 2) array of the volume's shape, uploaded for the call.  Returns the flood's stats."""
        self._materialize_mask()
        mk = np.ascontiguousarray(markers)
        if mk.shape != self.shape or mk.dtype.type not in (np.int8, np.int16):
            raise TypeError("markers must be an int8 / int16 array of the volume's shape")
        s3 = np.zeros((3, 3, 3), np.uint8)
        s3[:] = np.asarray(strct).astype(bool)
        lib, n = L.lib(), self.n
        d_mk, d_cost, d_lab = DeviceBuffer(mk.nbytes), DeviceBuffer(n * 2), DeviceBuffer(n)
        d_mk.upload(mk)
        try:
            if use_ww_wl:
                L.check(lib.ivx_dev_lut_u16(self.image.raw, c64(n), ctypes.c_double(float(ww)), ctypes.c_double(float(wl)), 0,
                                            d_cost.ptr, self.stream), "lut")
            else:
                mm = DeviceBuffer(64)
                L.check(lib.ivx_dev_minmax_f32(L.I16, self.image.raw, c64(n), mm.ptr, self.stream))
                self.sync()
                imin = int(mm.download((2,), np.float32)[0])
                mm.close()
                L.check(lib.ivx_dev_shift_min_u16(self.image.raw, c64(n), imin, d_cost.ptr, self.stream), "min shift")
            stats = (ctypes.c_int64 * 16)()
            mdt = L.I16 if mk.dtype == np.int16 else L.I8
            if algorithm == "Watershed":  # watershed_process.py:33-39,47-52
                d_grad = DeviceBuffer(n * 2)
                try:
                    gsz = (ctypes.c_int * 3)(*[int(v) for v in mg_size])
                    L.check(lib.ivx_dev_morph_gradient_u16(d_cost.ptr, c64(self.dz), c64(self.dy), c64(self.dx), gsz, d_grad.ptr,
                                                           self.stream), "gradient")
                    with self.timer.span("watershed_flood"):
                        L.check(lib.ivx_dev_watershed_sk(d_grad.ptr, mdt, d_mk.ptr, c64(self.dz), c64(self.dy), c64(self.dx), L.ptr(s3),
                                                         None, None, d_lab.ptr, None, stats, self.stream), "watershed_sk")
                    self.sync()
                finally:
                    d_grad.close()
            else:
                with self.timer.span("watershed_flood"):
                    L.check(lib.ivx_dev_watershed_ift(d_cost.ptr, mdt, d_mk.ptr, c64(self.dz), c64(self.dy), c64(self.dx), L.ptr(s3),
                                                      None, d_lab.ptr, None, stats, self.stream), "watershed_ift")
            L.check(lib.ivx_dev_watershed_merge(self.mask.ptr, d_lab.ptr, c64(n), int(bool(overwrite)), self.stream), "merge")
            self.sync()
        finally:
            for b in (d_mk, d_cost, d_lab):
                b.close()
        names = (("rounds", "tile_visits", "levels", "generations", "markers", "generation0", "tied_markers_of_different_labels")
                 if algorithm == "Watershed" else ("rounds", "tile_visits", "levels", "time_stamps", "markers", "entries", "tiles"))
        res = {k: int(v) for k, v in zip(names, stats)}
        if algorithm == "Watershed":
            from .watershed_process import _warn_ties
            _warn_ties(res["tied_markers_of_different_labels"], "DeviceVolume.watershed")
        return res

    # -- projections ---------------------------------------------------------------------------------
    def project(self, axis: int, op: int, out: DeviceBuffer):
        self._materialize_mask()
        L.check(L.lib().ivx_dev_mip_reduce(L.I16, self.image.raw, c64(self.dz), c64(self.dy), c64(self.dx), int(axis),
                                           int(op), out.ptr, self.stream), "project")

    def image_range(self) -> DeviceBuffer:
        """float32[2] on the device: min and max of the resident image -- mida_internal's own pre-pass over the volume
        (mips.rs:113-121).  The reference runs it inside every call; a resident volume keeps the result until the image's
        bytes change (any access to `image` from outside the pipeline's kernels drops it, like the bit-plane notes), the way
        `Slice` keeps the image's histogram (slice_.py:192-194; SURVEY 8d counts the cached range as allowed).
        `forget_image_range()` drops it by hand -- and every writer inside this package that goes to `image.raw` /
        `image.raw_at()` directly (past the tracked accessor) must call it -- or `_image_touched()`, which also drops the
        per-word records the threshold keeps (`_ranges`)."""
        self._materialize_mask()
        if getattr(self, "_range_buf", None) is None:
            self._range_buf = DeviceBuffer(64)
            self._range_valid = False
        if not self._range_valid:
            self._range_host = None  # (show_slice's host copy of the two numbers)
            L.check(L.lib().ivx_dev_minmax_f32(L.I16, self.image.raw, c64(self.n), self._range_buf.ptr, self.stream), "minmax")
            self._range_valid = True
        return self._range_buf

    def forget_image_range(self):
        self._materialize_mask()
        self._range_valid = False

    # -- image filters (filters.py via Slice.__apply_image_filter, slice_.py:2330-2430) ----------------------------------
    def filter_image(self, filter_type: int, value, dimension: str = "3D", orientation: str = "Axial"):
        """Replace the resident image by the dialog's filter `filter_type` (0 Gaussian, 1 median, 2 mean, 3 sharpen,
        4 despeckle, 5 border detection) with `value`, in HBM, no host round trip; ``dimension != "3D"`` filters every
        slice along the orientation's axis.  Everything derived from the image is dropped (``_image_touched``), so a
        threshold, region growing or surface after it works on the filtered image, as it does after _after_filter."""
        self._materialize_mask()
        from . import filters as F
        from .slice_ import _FILTER_PLANES

        if filter_type not in F.FILTER_NAMES:
            raise ValueError("unknown filter type %r" % (filter_type,))
        plane = -1 if dimension == "3D" else _FILTER_PLANES.get(orientation, 0)
        lib, shape = L.lib(), L.i64(self.shape)
        nb = ctypes.c_size_t(0)
        L.check(lib.ivx_filter_scratch_bytes(int(filter_type), shape, plane, ctypes.byref(nb)), "filter_scratch_bytes")
        self._join_prefetch()  # a surface count still reading the image must see the old one
        out, scratch = DeviceBuffer(self.n * 2), DeviceBuffer(nb.value)
        try:
            st, src = self.stream, self.image.raw
            if filter_type == F.MEDIAN:
                rc = lib.ivx_dev_filter_median_i16(src, shape, plane, F.median_size(value), out.ptr, st)
            elif filter_type == F.MEAN:
                rc = lib.ivx_dev_filter_mean_i16(src, shape, plane, F.mean_size(value), out.ptr, scratch.ptr, st)
            else:
                w, r = F.gaussian_weights(1.0 if filter_type == F.SHARPEN else value)
                if r > F.MAX_RADIUS:
                    raise ValueError("sigma %r needs a kernel radius of %d (at most %d)" % (value, r, F.MAX_RADIUS))
                wp = None if w is None else L.ptr(w)
                if filter_type == F.SHARPEN:
                    rc = lib.ivx_dev_filter_sharpen_i16(src, shape, plane, ctypes.c_double(float(value)), wp, int(r), out.ptr,
                                                        scratch.ptr, st)
                elif filter_type == F.BORDER:
                    rc = lib.ivx_dev_filter_border_i16(src, shape, plane, 1, wp, int(r), out.ptr, scratch.ptr, st)
                else:
                    rc = lib.ivx_dev_filter_gaussian_i16(src, shape, plane, wp, int(r), out.ptr, scratch.ptr, st)
            L.check(rc, "filter_image")
            L.check(lib.ivx_memcpy_d2d(self.image.ptr, out.ptr, ctypes.c_size_t(self.n * 2), st), "filter_image copy")
            self.sync()  # the buffers go out of scope here
        finally:
            out.close()
            scratch.close()
        self._image_touched()

    # -- deep-learning segmentation (segment_torch, segment.py:162-191; apply_segment_threshold, :465-490) -------------
    def segment_unet3d(self, weights, overlap: int = 50, patch_size: int = 48, apply_wwwl: bool = False, window_width=255,
                       window_level=127, batch: int | None = None) -> DeviceBuffer:
        """The U-Net segmentation of the resident image (get_LUT_value first if `apply_wwwl`) into the resident float32
        probability map `self.prob`, which is returned; `weights` as for segment.load_weights, or a segment.Unet3D.
        The image and the mask are left as they are: apply_segment_threshold writes the mask."""
        self._materialize_mask()
        from . import segment as SG

        SG._check_args(patch_size, overlap)
        net = weights if isinstance(weights, SG.Unet3D) else SG.Unet3D(weights)
        batch = SG.DEFAULT_BATCH if batch is None else int(batch)
        lib, st, n = L.lib(), self.stream, self.n
        if getattr(self, "prob", None) is None:
            self.prob = DeviceBuffer(n * 4)
        ws, norm, small = DeviceBuffer(net.workspace_bytes(patch_size, batch)), DeviceBuffer(n * 4), DeviceBuffer(64)
        lut = DeviceBuffer(n * 2) if apply_wwwl else None
        try:
            src = self.image.raw
            if apply_wwwl:  # get_LUT_value keeps int16 (np.piecewise)
                L.check(lib.ivx_dev_lut_i16(src, c64(n), ctypes.c_double(float(window_width)),
                                            ctypes.c_double(float(window_level)), 0, lut.ptr, st), "segment lut")
                src = lut.ptr
            L.check(lib.ivx_dev_unet3d_normalize(src, c64(n), norm.ptr, small.ptr, st), "segment normalize")
            self.prob.zero(st)
            L.check(lib.ivx_dev_unet3d_segment(net.handle, norm.ptr, L.i64(self.shape), int(patch_size), int(overlap), batch,
                                               self.prob.ptr, ws.ptr, ctypes.c_size_t(ws.nbytes), None, st), "segment_unet3d")
            self.sync()  # the buffers go out of scope here
        finally:
            for b in (ws, norm, small, lut):
                if b is not None:
                    b.close()
        return self.prob

    def apply_segment_threshold(self, threshold: float):
        """mask.matrix[1:, 1:, 1:] = (prob >= float32(threshold)) * 255 on the resident mask: one kernel per slider move;
        marching_cubes follows without an upload.  The per-slice flag lines live in the host mask's border
        (segment.apply_segment_threshold writes them there)."""
        self._materialize_mask()
        if getattr(self, "prob", None) is None:
            raise RuntimeError("apply_segment_threshold: no probability map (run segment_unet3d first)")
        L.check(L.lib().ivx_dev_segment_threshold(self.prob.ptr, L.i64(self.shape), ctypes.c_float(float(threshold)),
                                                  self.mask.ptr, L.i64([self.dy * self.dx, self.dx, 1]), 0, self.stream),
                "segment_threshold")

    # -- volume rendering (Volume.LoadVolume, volume.py:575-707; CalculateHistogram, :723-735) ---------------------------
    def _drop_volren(self, all_buffers: bool = False):
        """The prepared field and its macro cells depend on the image; the table, output and stats buffers do not."""
        vr = getattr(self, "_vr", None)
        if vr is not None:
            for b in (vr["vol"], vr["cells"]):
                b.close()
            self._vr = None
        if all_buffers:
            for name in ("_vr_table", "_vr_out", "_vr_stats"):
                b = getattr(self, name, None)
                if b is not None:
                    b.close()
                setattr(self, name, None)

    def _image_scale(self):
        """(min, max) of the resident image as integers (GetScalarRange of LoadVolume)"""
        rng = np.empty(2, np.float32)
        buf = self.image_range()
        self.sync()
        buf.download((2,), np.float32, rng)
        return int(rng[0]), int(rng[1])

    def _volren_field(self, shift: int, kernels) -> dict:
        """The prepared uint16 field (shift + the preset's smoothing passes) and its macro cells, kept per (shift, filter
        list) until the image changes: a camera move or a WW/WL change only re-bakes the table."""
        from . import volume as V

        key = (int(shift), len(kernels))
        vr = getattr(self, "_vr", None)
        if vr is not None and vr["key"] == key:
            return vr
        self._drop_volren()
        cshape = [-(-s // V.CELL) for s in self.shape]
        vol, cells = DeviceBuffer(self.n * 2), DeviceBuffer(int(np.prod(cshape)) * 4)
        scratch = DeviceBuffer(self.n * 2) if kernels else None
        try:
            lib, shape = L.lib(), L.i64(self.shape)
            L.check(lib.ivx_dev_volren_prepare(self.image.raw, shape, int(shift), len(kernels), vol.ptr,
                                               None if scratch is None else scratch.ptr, self.stream), "volren_prepare")
            L.check(lib.ivx_dev_volren_cells(vol.ptr, shape, cells.ptr, self.stream), "volren_cells")
            self.sync()  # scratch goes out of scope here
        except Exception:
            vol.close()
            cells.close()
            raise
        finally:
            if scratch is not None:
                scratch.close()
        self._vr = {"key": key, "vol": vol, "cells": cells, "cshape": cshape}
        return self._vr

    @staticmethod
    def _grow(owner, name, nbytes):
        b = getattr(owner, name, None)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.close()
            b = DeviceBuffer(nbytes)
            setattr(owner, name, b)
        return b

    def _render(self, bufs: str, size, rgba8: bool, depth: bool, download: bool, launch):
        """What the two renders share: grow the `bufs`_out and _stats (with `depth` also _depth) buffers, zero the
        counters and `launch(out, depth buffer or None, stats)`; then return the device buffer(s), or with `download`
        sync, leave the sample counts in ``last_render_stats`` and return the arrays."""
        w, h = size
        out = self._grow(self, bufs + "_out", w * h * 4 * (1 if rgba8 else 4))
        dep = self._grow(self, bufs + "_depth", w * h * 4) if depth else None
        stats = self._grow(self, bufs + "_stats", 32)
        stats.zero(self.stream, 32)
        launch(out, dep, stats)
        if download:
            self.sync()
            st = stats.download((4,), np.uint64)
            self.last_render_stats = {"samples": int(st[0]), "skipped": int(st[1]), "early": int(st[2]),
                                      "rays_hit": int(st[3]), "rays": w * h}
            out = out.download((h, w, 4), np.uint8 if rgba8 else np.float32)
            dep = dep.download((h, w), np.float32) if depth else None
        return (out, dep) if depth else out

    def render_volume(self, preset, camera, size, clip_plane=None, shade=None, color_lists=None, download: bool = True,
                      rgba8: bool = False, presets_dir=None):
        """The 3-D view of the resident image with a raycasting preset (a dict, a .plist path, or a name in
        `presets_dir`).  `camera`: a standard view name ("front", "back", "left", "right", "top", "bottom", "iso") or a
        dict from volume.camera_for_view; `size` (width, height) in pixels.  `shade` None follows the preset's useShading
        (see volume.shading).  Returns (height, width, 4) float32 RGBA (uint8 with `rgba8`), or the device buffer when not
        `download`.  The sample counts are left in ``last_render_stats`` by a downloading render; without `download`
        nothing is waited for, so they stay those of the last render that did."""
        self._materialize_mask()
        from . import volume as V

        cam = V.resolve_camera(camera, self.shape, self.spacing, size)
        scale = self._image_scale()
        setup = V.render_setup(preset, scale, cam, clip_plane, shade, color_lists, presets_dir)
        vr = self._volren_field(setup["shift"], setup["kernels"])
        rgba, alpha, prefix = V.device_tables(setup)
        tb = self._grow(self, "_vr_table", rgba.nbytes + alpha.nbytes + prefix.nbytes)
        self.sync()  # the table buffer may still be read by the previous render
        host = np.concatenate([rgba.view(np.uint8).ravel(), alpha.view(np.uint8).ravel(), prefix.view(np.uint8).ravel()])
        tb.upload(host)
        p = V.volren_params(setup, self.spacing, rgba8)

        def launch(out, dep, stats):
            L.check(L.lib().ivx_dev_volren_render(vr["vol"].ptr, vr["cells"].ptr, L.i64(self.shape), tb.ptr,
                                                  tb.at(rgba.nbytes), tb.at(rgba.nbytes + alpha.nbytes), ctypes.byref(p),
                                                  out.ptr, stats.ptr, self.stream), "render_volume")
            self._vr_setup = setup

        return self._render("_vr", cam["viewport"], rgba8, False, download, launch)

    # -- mask 3-D preview (VolumeMask.create_volume, volume_mask.py:36-119) ----------------------------------------------
    def _drop_maskren(self):
        for name in ("_mp_cells", "_mp_table", "_mp_out", "_mp_depth", "_mp_stats"):
            b = getattr(self, name, None)
            if b is not None:
                b.close()
            setattr(self, name, None)
        self._mp_cells_valid = False
        self._mp_table_key = None

    def _maskren_cells(self, apron_value: int) -> DeviceBuffer:
        """The macro cells of the resident mask with its virtual flag planes, kept until the mask's bytes change
        (``_mp_cells_valid`` is dropped by everything that writes them) or another apron value is asked for."""
        from . import volume as V

        key = int(apron_value)
        self._materialize_mask()  # (the cells are made from the bytes, and the render reads them)
        if getattr(self, "_mp_cells_valid", False) and self._mp_cells_key == key:
            return self._mp_cells
        ncell = int(np.prod([-(-(s + 1) // V.CELL) for s in self.shape]))
        cells = self._grow(self, "_mp_cells", ncell * 2)
        L.check(L.lib().ivx_dev_maskren_cells(self.mask.raw, L.i64(self.shape), L.i64([self.dy * self.dx, self.dx, 1]), 1,
                                              key, c64(0), c64(-1), cells.ptr, self.stream), "maskren_cells")
        self._mp_cells_valid, self._mp_cells_key = True, key
        return cells

    def render_mask_preview(self, colour, camera, size, mode: str = "composite", apron_value: int = 1,
                            download: bool = True, rgba8: bool = False, depth: bool = False, background=(0.0, 0.0, 0.0),
                            sample_distance=None):
        """The 3-D preview of the resident mask (volume_mask.render_setup: `mode` "composite" or "iso", `colour` r, g, b in
        0..1), read in place.  The mask is dense, so the index-0 flag planes of the reference's matrix are a virtual apron
        of `apron_value` (1 is what a whole-volume threshold leaves there).  `camera`: a standard view name or a dict from
        volume.camera_for_view; `size` (width, height).  Returns (height, width, 4) float32 RGBA (uint8 with `rgba8`),
        with `depth` (iso mode) also the (height, width) float32 distance of the hit, or the device buffer(s) when not
        `download`.  The sample counts are left in ``last_render_stats`` by a downloading render; without `download`
        nothing is waited for, so they stay those of the last render that did."""
        self._materialize_mask()
        from . import volume as V
        from . import volume_mask as VM

        if depth and mode != "iso":
            raise ValueError("depth is an output of the iso mode")
        cam = V.resolve_camera(camera, self.shape, self.spacing, size)
        setup = VM.render_setup(colour, mode, cam, self.spacing, background, sample_distance)
        rgba, prefix = VM.device_tables(setup)
        cells = self._maskren_cells(apron_value)
        tb = self._grow(self, "_mp_table", rgba.nbytes + prefix.nbytes)
        key = (tuple(float(c) for c in colour), mode, setup["dt"])
        if getattr(self, "_mp_table_key", None) != key:  # a slider step or a camera move keeps the table: no stall
            self.sync()  # the table buffer may still be read by the previous render
            tb.upload(np.concatenate([rgba.view(np.uint8).ravel(), prefix.view(np.uint8).ravel()]))
            self._mp_table_key = key
        p = V.volren_params(setup, self.spacing, rgba8)

        def launch(out, dep, stats):
            L.check(L.lib().ivx_dev_maskren_render(self.mask.raw, cells.ptr, L.i64(self.shape),
                                                   L.i64([self.dy * self.dx, self.dx, 1]), 1, int(apron_value),
                                                   int(setup["iso"]), tb.ptr, tb.at(rgba.nbytes), ctypes.byref(p), out.ptr,
                                                   None if dep is None else dep.ptr, stats.ptr, self.stream),
                    "render_mask_preview")

        return self._render("_mp", cam["viewport"], rgba8, depth, download, launch)

    def render_scene(self, camera, size, surfaces=None, planes=(), **kw):
        """The 3-D view with everything in it (scene3d.Scene3D.render): the resident image under a composite
        `preset=` or the resident mask in `mask_colour=`, with `surfaces` (a surface_view.Scene or SurfaceActors) and `planes`
        (scene3d.SlicePlanes) blended at their depths.  The scene is kept for the next call with the same `surfaces` object
        and `planes`, so its key buffers and pictures stay resident."""
        from . import scene3d as S3

        sc = getattr(self, "_scene3d", None)
        if sc is None or sc[0] is not surfaces:
            if sc is not None:
                sc[1].close()
            sc = self._scene3d = (surfaces, S3.Scene3D(self, surfaces))
        sc[1].planes = list(planes)
        out = sc[1].render(camera, size, **kw)
        self.last_render_stats = sc[1].last_render_stats if kw.get("download", True) else self.last_render_stats
        return out

    def volume_histogram(self) -> np.ndarray:
        """CalculateHistogram (volume.py:723-735) of the resident image: uint64 counts of the int(max - min) unit bins
        from min (voxels equal to max are not counted; a constant image gives an empty histogram)."""
        self._materialize_mask()
        lo, hi = self._image_scale()
        nb = hi - lo
        if nb <= 0:
            return np.zeros(0, np.uint64)
        counts = DeviceBuffer(nb * 8)
        try:
            L.check(L.lib().ivx_dev_volren_histogram(self.image.raw, c64(self.n), int(lo), int(nb), counts.ptr, self.stream),
                    "volume_histogram")
            self.sync()
            return counts.download((nb,), np.uint64)
        finally:
            counts.close()

    def mida(self, axis: int, wl, ww, out: DeviceBuffer, status: DeviceBuffer):
        """mida (mips.rs:102-168) of the resident image along `axis` into `out` (int16 image of the projection's shape); the
        volume's range comes from `image_range()`.  `status` (int32, zeroed by the caller) receives IVX_EDOM where the
        reference's NumCast would panic.  Window level / width are truncated like the reference's wrapper does
        (invesalius_rs/__init__.py:91-95: ``_native.mida(image, axis, int(wl), int(ww), out)``)."""
        self._materialize_mask()
        L.check(L.lib().ivx_dev_mida(L.I16, self.image.raw, c64(self.dz), c64(self.dy), c64(self.dx), int(axis), ctypes.c_float(float(int(wl))),
                                     ctypes.c_float(float(int(ww))), self.image_range().ptr, L.I16, out.ptr, status.ptr, self.stream), "mida")


def c64(v):
    return ctypes.c_int64(int(v))
