"""The mask edit history: Edit -> Undo / Redo of mask edits, with the states kept in HBM.

`EditionHistory` restates the bookkeeping of the reference's class of the same name (invesalius/data/mask.py:78-203) rule
for rule -- capacity, truncation of the redo tail, the VOLUME branch, the scroll-only step, the double step and the
``Enable undo`` / ``Enable redo`` messages -- while the nodes hold device blocks instead of ``.npy`` temporary files:

* a VOLUME node holds a `Snapshot`, the whole padded matrix in the `blocks64` format (csrc/k_maskhist.hip).  Committing it
  restores the bound matrix's mirror in place and downloads only the planes that changed; an unbound matrix is decoded and
  downloaded whole;
* a slice node (AXIAL / CORONAL / SAGITAL) holds its ``h x w`` bytes raw, and commits through the device-block route of
  `slice_.apply_slice_buffer_to_mask`, so that host and mirror receive the same bytes.

    p = history.snapshot(matrix)                 # before the tool; from the mirror when the matrix is bound
    styles.crop_mask(matrix, image, limits)
    h.new_node(0, "VOLUME", history.snapshot(matrix), p, False)      # no mask byte has crossed the link
    ...
    h.undo(matrix, actual_slices)                # mirror restored, the changed planes downloaded

or ``with history.recorded(h, matrix) as rec: rec.result = mask.fill_holes_auto(matrix, ...)``.

One deviation from the reference: `undo` / `redo` on an empty history do nothing (the reference dies with IndexError in its
trace ``print``).  Still with the caller: the GUI's menu enabling (the messages are handed to `publish`),
``session.ChangeProject`` and the reference's temporary files."""
from __future__ import annotations

import ctypes
from contextlib import contextmanager

import numpy as np

from . import _lib as L
from . import slice_ as sl
from .device import DeviceBuffer

VOLUME = "VOLUME"
_live_blocks = 0


def live_device_blocks() -> int:
    """device blocks the histories and snapshots of this process hold at the moment"""
    return _live_blocks


class _Block(DeviceBuffer):
    """a DeviceBuffer the module counts (live_device_blocks); `adopt` wraps a block the library allocated"""

    def __init__(self, nbytes: int):
        global _live_blocks
        super().__init__(nbytes)
        _live_blocks += 1

    @classmethod
    def adopt(cls, ptr, nbytes: int) -> "_Block":
        global _live_blocks
        b = cls.__new__(cls)
        b.nbytes, b.ptr = int(nbytes), ctypes.c_void_p(ptr)
        _live_blocks += 1
        return b

    def close(self):
        global _live_blocks
        if getattr(self, "ptr", None) is not None and self.ptr.value:
            _live_blocks -= 1
        super().close()


def header_bytes(n: int) -> int:
    out = ctypes.c_size_t(0)
    L.check(L.lib().ivx_mask_snapshot_header_bytes(int(n), ctypes.byref(out)), "snapshot header")
    return int(out.value)


class Snapshot:
    """One encoded state of a byte volume: `header` and `pool` (DeviceBuffers), `n` bytes of `shape`, `literal_blocks`
    blocks of 64 bytes in the pool.  A node that is given a Snapshot owns it from then on and frees it when it leaves the
    history; the same Snapshot may serve several nodes and goes with the last one."""

    def __init__(self, header: DeviceBuffer, pool: DeviceBuffer, n: int, shape, literal_blocks: int):
        self.header, self.pool, self.n, self.shape = header, pool, int(n), tuple(int(s) for s in shape)
        self.literal_blocks = int(literal_blocks)
        self._owners = 0

    @property
    def device_bytes(self) -> int:
        return header_bytes(self.n) + 64 * self.literal_blocks

    @property
    def closed(self) -> bool:
        return self.header is None

    def close(self):
        for b in (self.header, self.pool):
            if b is not None:
                b.close()
        self.header = self.pool = None

    def _disown(self):
        self._owners -= 1
        if self._owners <= 0:
            self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _dense_u8(matrix, what):
    if not isinstance(matrix, np.ndarray) or matrix.dtype != np.uint8 or not matrix.flags["C_CONTIGUOUS"] or matrix.size == 0:
        raise TypeError("%s: a C-contiguous, non-empty uint8 array" % what)
    return matrix


def snapshot(matrix: np.ndarray) -> Snapshot:
    """Encode the padded host matrix.  A matrix bound with `mask.bind_matrix` is read from its mirror -- nothing crosses the
    link; any other array is uploaded once."""
    m = _dense_u8(matrix, "history.snapshot")
    L.require_device()
    hdr, pool, nlit = ctypes.c_void_p(), ctypes.c_void_p(), L.c_i64(0)
    L.check(L.lib().ivx_mask_snapshot(L.ptr(m), m.nbytes, ctypes.byref(hdr), ctypes.byref(pool), ctypes.byref(nlit)), "history.snapshot")
    return Snapshot(_Block.adopt(hdr.value, header_bytes(m.nbytes)), _Block.adopt(pool.value, max(64 * nlit.value, 16)), m.nbytes, m.shape,
                    nlit.value)


def snapshot_device(src, n: int, shape, stream=None) -> Snapshot:
    """Encode `n` bytes of device memory at `src` on `stream` (what DeviceVolume.snapshot_mask does with its mask)."""
    header = _Block(header_bytes(n))
    pool = None
    try:
        nlit = L.c_i64(0)
        L.check(L.lib().ivx_dev_mask_snapshot_scan(src, int(n), header.ptr, ctypes.byref(nlit), stream), "snapshot scan")
        pool = _Block(max(64 * nlit.value, 16))
        L.check(L.lib().ivx_dev_mask_snapshot_pack(src, int(n), header.ptr, pool.ptr, nlit.value, stream), "snapshot pack")
        L.check(L.lib().ivx_stream_synchronize(stream), "snapshot pack")  # (a snapshot may be restored on another stream)
    except Exception:
        header.close()
        if pool is not None:
            pool.close()
        raise
    return Snapshot(header, pool, n, shape, nlit.value)


def restore(snap: Snapshot, matrix: np.ndarray) -> int:
    """``matrix[:] = the snapshot's state``, host and mirror alike.  Returns the planes (``matrix[i]``) written on the
    host: those that changed when the matrix is bound, all of them otherwise."""
    if snap.closed:
        raise ValueError("history.restore: the snapshot has been closed")
    m = _dense_u8(matrix, "history.restore")
    if tuple(m.shape) != snap.shape:
        raise ValueError("history.restore: the snapshot holds shape %r, the matrix has %r" % (snap.shape, tuple(m.shape)))
    plane = m.nbytes // m.shape[0]
    written = L.c_i64(0)
    L.check(L.lib().ivx_mask_snapshot_restore(L.ptr(m), m.nbytes, snap.header.ptr, snap.pool.ptr, snap.literal_blocks, plane,
                                              ctypes.byref(written)), "history.restore")
    return int(written.value)


class _VolumeNode:
    def __init__(self, index, orientation, array, clean):
        self.index, self.orientation, self.clean = index, orientation, clean
        if isinstance(array, Snapshot):
            if array.closed:
                raise ValueError("EditionHistory: the snapshot has been closed")
            self.snapshot = array
        else:
            self.snapshot = snapshot(np.ascontiguousarray(array, dtype=np.uint8))  # the reference's call surface: one staged upload
        self.snapshot._owners += 1

    def commit_history(self, mvolume):
        restore(self.snapshot, mvolume)

    def release(self):
        if self.snapshot is not None:
            self.snapshot._disown()
            self.snapshot = None


class _SliceNode:
    def __init__(self, index, orientation, array, clean):
        sl._axis(orientation)
        if isinstance(array, Snapshot):
            raise TypeError("EditionHistory: a %s node takes the slice's array, a Snapshot belongs to a VOLUME node" % orientation)
        a = np.ascontiguousarray(array, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("EditionHistory: a slice node takes a 2-D array")
        self.index, self.orientation, self.clean, self.shape = index, orientation, clean, a.shape
        self.buf = _Block(a.size + 16)
        self.buf.upload(np.concatenate([a.reshape(-1), np.array([1], np.uint8)]))  # the slice, then the byte `clean` writes

    def commit_history(self, mvolume):
        mview, flag, _ = sl._slice_views(mvolume, None, self.orientation, self.index)
        if mview.shape != self.shape:
            raise ValueError("EditionHistory: the node holds a slice of shape %r, the mask's slice has %r" % (self.shape, mview.shape))
        self.buf.download_view(mview)  # host and mirror, these bytes alone
        if self.clean:
            n = self.shape[0] * self.shape[1]
            L.check(L.lib().ivx_download_strided(L.ptr(flag), L.i64((1, 1, 1)), L.i64((1, 1, 1)), self.buf.at(n), 1), "commit_history")

    def release(self):
        if self.buf is not None:
            self.buf.close()
            self.buf = None


def _node(index, orientation, array, clean):
    return (_VolumeNode if orientation == VOLUME else _SliceNode)(index, orientation, array, clean)


class EditionHistory:
    """`size` undo steps: up to ``size * 2`` nodes (every edit stores the state before and the state after).
    `publish(topic, **kw)` receives what the reference sends through its Publisher."""

    def __init__(self, size: int = 50, publish=None):
        self.history = []
        self.index = -1
        self.size = size * 2
        self._publish = publish
        self._send("Enable undo", value=False)
        self._send("Enable redo", value=False)

    def _send(self, topic, **kw):
        if self._publish is not None:
            self._publish(topic, **kw)

    def new_node(self, index, orientation, array, p_array, clean):
        """an edit of slice `index` of `orientation` (or 0, "VOLUME"): `p_array` the state before, `array` the state after"""
        before = _node(index, orientation, p_array, clean)
        try:
            after = _node(index, orientation, array, clean)
        except Exception:
            before.release()
            raise
        self.add(before)
        self.add(after)

    def add(self, node):
        if self.index == self.size:  # full: the oldest node goes
            self.history.pop(0).release()
            self.index -= 1
        if self.index < len(self.history):  # a new edit after undos: the redo tail goes
            for dropped in self.history[self.index + 1:]:
                dropped.release()
            del self.history[self.index + 1:]
        self.history.append(node)
        self.index += 1
        self._send("Enable undo", value=True)
        self._send("Enable redo", value=False)

    def _shown_elsewhere(self, node, actual_slices):
        return bool(actual_slices) and actual_slices[node.orientation] != node.index

    def _shown_here(self, node, actual_slices):
        return bool(actual_slices) and actual_slices[node.orientation] == node.index

    def _move(self, step, mvolume):
        self.index += step
        self.history[self.index].commit_history(mvolume)

    def undo(self, mvolume, actual_slices=None):
        h = self.history
        if not h:
            return
        if self.index > 0:
            target = h[self.index - 1]
            if target.orientation != VOLUME and self._shown_elsewhere(target, actual_slices):
                self._reload_slice(self.index - 1)  # the viewer shows another slice: scroll there, change nothing
            else:
                self._move(-1, mvolume)
                if target.orientation != VOLUME and self.index and self._shown_here(h[self.index - 1], actual_slices):
                    self._move(-1, mvolume)  # the next node lies on the shown slice too: the pair in one step
                self._reload_slice(self.index)
                self._send("Enable redo", value=True)
        if self.index == 0:
            self._send("Enable undo", value=False)

    def redo(self, mvolume, actual_slices=None):
        h = self.history
        if not h:
            return
        if self.index < len(h) - 1:
            target = h[self.index + 1]
            if target.orientation != VOLUME and self._shown_elsewhere(target, actual_slices):
                self._reload_slice(self.index + 1)
            else:
                self._move(+1, mvolume)
                if target.orientation != VOLUME and self.index < len(h) - 1 and self._shown_here(h[self.index + 1], actual_slices):
                    self._move(+1, mvolume)
                self._reload_slice(self.index)
                self._send("Enable undo", value=True)
        if self.index == len(h) - 1:
            self._send("Enable redo", value=False)

    def _reload_slice(self, index):
        node = self.history[index]
        self._send(("Set scroll position", node.orientation), index=node.index)

    def _config_undo_redo(self, visible):
        v_undo = v_redo = False
        if self.history and visible:
            v_undo = v_redo = True
            if self.index == 0:
                v_undo = False
            elif self.index == len(self.history) - 1:
                v_redo = False
        self._send("Enable undo", value=v_undo)
        self._send("Enable redo", value=v_redo)

    def clear_history(self):
        for node in self.history:
            node.release()
        self.history = []
        self.index = -1
        self._send("Enable undo", value=False)
        self._send("Enable redo", value=False)

    def device_bytes(self) -> int:
        """HBM the nodes hold"""
        seen, total = set(), 0
        for node in self.history:
            if isinstance(node, _VolumeNode):
                if id(node.snapshot) not in seen:
                    seen.add(id(node.snapshot))
                    total += node.snapshot.device_bytes
            else:
                total += node.buf.nbytes
        return total


class _Recording:
    """what `recorded` yields: set `result` to the tool's return value (False: nothing changed, no node is added)"""
    result = None


@contextmanager
def recorded(history: EditionHistory, matrix: np.ndarray, index=0, orientation=VOLUME, clean=False):
    """Record one whole-matrix tool: a snapshot before, one after when the tool did not raise, and the node pair -- unless
    the tool reported through ``rec.result = tool(...)`` that it changed nothing (the tools that return ``bool``)."""
    if orientation != VOLUME:
        raise ValueError("history.recorded: whole-matrix tools only (a slice tool hands its slices to new_node)")
    before = snapshot(matrix)
    rec = _Recording()
    try:
        yield rec
    except BaseException:
        before.close()
        raise
    if rec.result is False:
        before.close()
        return
    try:
        after = snapshot(matrix)
    except Exception:
        before.close()
        raise
    history.new_node(index, orientation, after, before, clean)
