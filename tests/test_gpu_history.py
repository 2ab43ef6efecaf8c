"""GPU: the mask edit history (invesalius3_amd/history.py) against the reference's own EditionHistory
(tests/golden/ref_history.npz) on unbound and bound matrices, what it moves across the link, what it keeps alive, and the
DeviceVolume forms."""
import numpy as np
import pytest

import _history_ref as R
from conftest import synth_volume

pytestmark = pytest.mark.gpu


def _bound_write(view, array):
    from invesalius3_amd import resident
    view[...] = array
    resident.touch(view)  # a numpy write of a bound matrix is followed by a touch (the "tool" of the scripts is numpy)


def _snap_wrap(array, matrix, orientation):
    from invesalius3_amd import history
    return history.snapshot(matrix) if orientation == "VOLUME" else array


@pytest.mark.parametrize("snapshots", (False, True), ids=("arrays", "snapshots"))
@pytest.mark.parametrize("name", R.script_names())
def test_scripts_equal_the_reference_unbound(ivxlib, name, snapshots):
    from invesalius3_amd import history
    live = history.live_device_blocks()
    m = np.zeros(R.fixture()["init_" + name].shape, np.uint8)
    h = R.replay(name, lambda size, publish: history.EditionHistory(size, publish), m, wrap=_snap_wrap if snapshots else None)
    h.clear_history()
    assert history.live_device_blocks() == live


@pytest.mark.parametrize("snapshots", (False, True), ids=("arrays", "snapshots"))
@pytest.mark.parametrize("name", R.script_names())
def test_scripts_equal_the_reference_bound_with_the_stale_check(ivxlib, name, snapshots):
    from invesalius3_amd import history, resident, slice_
    from invesalius3_amd import mask as mk
    m = np.zeros(R.fixture()["init_" + name].shape, np.uint8)
    with mk.bind_matrix(m):
        resident.set_check(True)  # every use compares host and mirror first: a mirror that fell behind raises
        try:
            h = R.replay(name, lambda size, publish: history.EditionHistory(size, publish), m, write=_bound_write,
                         wrap=_snap_wrap if snapshots else None)
            slice_.project(m, 0, slice_.PROJECTION_MaxIP)  # one more use of the whole matrix
        finally:
            resident.set_check(False)
        h.clear_history()


def _moved(before):
    from invesalius3_amd import resident
    now = resident.transfer_stats()
    return now["h2d_bytes"] - before["h2d_bytes"], now["d2h_bytes"] - before["d2h_bytes"]


def test_counters_on_a_bound_matrix(ivxlib):
    from invesalius3_amd import history, resident
    from invesalius3_amd import mask as mk
    rng = np.random.default_rng(3)
    m = np.array([0, 1, 254, 255], np.uint8)[rng.integers(0, 4, (9, 40, 33))]
    first = m.copy()
    with mk.bind_matrix(m) as rm:
        h = history.EditionHistory()
        # a VOLUME pair saved from Snapshots: nothing crosses the link in either direction
        s0 = resident.transfer_stats()
        p = history.snapshot(m)
        m[2, 5:9, 4:20] = 7
        m[3, 0, 0] = 7
        m[7, 39, 32] = 7
        rm.touch(m[2:8])  # (the tool's own upload, before the counters are read)
        history.snapshot(m).close()
        s1 = resident.transfer_stats()
        after = history.snapshot(m)
        h.new_node(0, "VOLUME", after, p, False)
        assert _moved(s1) == (0, 0)
        assert after.device_bytes == history.header_bytes(m.nbytes) + 64 * after.literal_blocks == h.device_bytes() - p.device_bytes
        edited = m.copy()
        # an undo that differs in 3 planes: 0 bytes up, exactly those planes down
        s2 = resident.transfer_stats()
        h.undo(m, {"AXIAL": 0, "CORONAL": 0, "SAGITAL": 0, "VOLUME": 0})
        assert _moved(s2) == (0, 3 * 40 * 33)
        assert np.array_equal(m, first)
        # an undo / redo onto an identical state moves nothing
        h.redo(m, None)
        assert np.array_equal(m, edited)
        s3 = resident.transfer_stats()
        h.undo(m, None)
        h.redo(m, None)
        h.redo(m, None)
        assert _moved(s3) == (0, 2 * 3 * 40 * 33) and np.array_equal(m, edited)
        s4 = resident.transfer_stats()
        history.restore(after, m)
        assert _moved(s4) == (0, 0)
        # a sagittal slice node's commit moves one slice
        before = m[1:, 1:, 6].copy()
        m[1:, 1:, 6] = 254
        rm.touch(m[1:, 1:, 6])
        h.new_node(5, "SAGITAL", m[1:, 1:, 6].copy(), before, False)
        history.snapshot(m).close()  # (the touched slice goes up here, before the counters are read)
        resident.set_check(True)
        try:
            s5 = resident.transfer_stats()
            h.undo(m, None)
            assert _moved(s5) == (0, 8 * 39)
            assert np.array_equal(m[1:, 1:, 6], before)
            history.snapshot(m).close()  # (reads the whole mirror under the stale check)
        finally:
            resident.set_check(False)
        _ = s0
        h.clear_history()
    # the same matrix unbound: there is nothing to compare with, so every plane comes down
    snap = history.snapshot(first)
    other = np.zeros_like(first)
    assert history.restore(snap, other) == 9 and np.array_equal(other, first)
    with pytest.raises(ValueError):
        history.restore(snap, np.zeros((9, 33, 40), np.uint8))
    snap.close()
    with pytest.raises(ValueError):
        history.restore(snap, other)


def test_nodes_that_leave_free_their_blocks(ivxlib):
    from invesalius3_amd import history
    live = history.live_device_blocks()
    m = np.zeros((6, 7, 8), np.uint8)
    h = history.EditionHistory(size=2)
    per_volume_pair, per_slice_pair = 4, 2
    h.new_node(0, "VOLUME", m.copy(), m.copy(), False)
    assert history.live_device_blocks() == live + per_volume_pair
    h.new_node(1, "AXIAL", m[2, 1:, 1:].copy(), m[2, 1:, 1:].copy(), True)
    assert history.live_device_blocks() == live + per_volume_pair + per_slice_pair
    h.new_node(0, "VOLUME", history.snapshot(m), history.snapshot(m), False)  # five nodes fit (size * 2 + 1), the oldest left
    assert len(h.history) == 5 and history.live_device_blocks() == live + 2 + per_slice_pair + per_volume_pair
    h.undo(m)
    h.undo(m)
    h.undo(m)
    h.new_node(1, "AXIAL", m[2, 1:, 1:].copy(), m[2, 1:, 1:].copy(), False)  # truncation: the three undone nodes go
    assert len(h.history) == 4 and history.live_device_blocks() == live + 2 + 1 + per_slice_pair
    shared = history.snapshot(m)
    h.new_node(0, "VOLUME", shared, shared, False)  # one Snapshot in two nodes goes with the last of them
    h.clear_history()
    assert shared.closed and history.live_device_blocks() == live and h.index == -1
    stray = history.snapshot(m)
    with pytest.raises(TypeError):
        h.new_node(1, "AXIAL", stray, m[2, 1:, 1:], False)
    stray.close()
    h.new_node(0, "VOLUME", np.zeros((5, 7, 8), np.uint8), m, False)
    h.undo(m)
    with pytest.raises(ValueError):  # a wrong shape
        h.redo(m)
    h.clear_history()
    import gc
    gc.collect()
    assert history.live_device_blocks() == live
    # an empty history: nothing happens (the reference dies in its trace print)
    sent = []
    e = history.EditionHistory(publish=lambda *a, **k: sent.append(a))
    del sent[:]
    e.undo(m)
    e.redo(m)
    assert not sent and e.index == -1


def test_recorded_tools(ivxlib):
    from invesalius3_amd import history, styles
    from invesalius3_amd import mask as mk
    image = synth_volume((12, 30, 34))
    m = np.zeros((13, 31, 35), np.uint8)
    m[1:, 1:, 1:] = np.where(image > 226, 255, 0)
    m[1:, 0, 0] = 1
    m[0, 1:, 0] = 1
    solid = m.copy()
    solid[1:, 1:, 1:] = 255
    for bound in (False, True):
        h = history.EditionHistory()
        a = solid.copy()
        binding = mk.bind_matrix(a) if bound else None
        with history.recorded(h, a) as rec:  # a solid mask has no holes: fill_holes_auto reports False, no node
            rec.result = mk.fill_holes_auto(a, "3D", 6, "AXIAL", 0, 1000)
        assert rec.result is False and h.index == -1 and not h.history
        if binding:
            binding.release()
        a = m.copy()
        binding = mk.bind_matrix(a) if bound else None
        with history.recorded(h, a):
            styles.crop_mask(a, None, (3, 20, 2, 17, 1, 6))
        cropped = a.copy()
        assert h.index == 1 and len(h.history) == 2 and not np.array_equal(cropped, m)
        assert (cropped[0] == 1).all()  # (the crop writes the flag planes too)
        mk.undo_history(a, h, {"AXIAL": 0, "CORONAL": 0, "SAGITAL": 0, "VOLUME": 0})
        assert np.array_equal(a, m)  # the bytes from before, flag planes included
        mk.redo_history(a, h)
        assert np.array_equal(a, cropped)
        with pytest.raises(RuntimeError):
            with history.recorded(h, a):
                raise RuntimeError("the tool failed")
        assert len(h.history) == 2
        mk.save_history(a, h, 0, "VOLUME", a.copy(), m.copy())
        assert len(h.history) == 4
        h.clear_history()
        if binding:
            binding.release()


def test_device_volume_snapshot_and_restore(ivxlib):
    from invesalius3_amd import history
    from invesalius3_amd.device import DeviceVolume
    from invesalius3_amd.mask import _structure
    image = synth_volume((20, 64, 64))  # (rows of whole 64-voxel words: the threshold defers the mask's bytes)
    seed = tuple(int(v) for v in np.unravel_index(int(np.argmax(image)), image.shape))[::-1]
    live = history.live_device_blocks()
    with DeviceVolume(image) as vol:
        vol.threshold(226, 3071)
        snap = vol.snapshot_mask()
        first = vol.download_mask().copy()
        assert np.array_equal(first, np.where(image >= 226, 255, 0).astype(np.uint8))
        assert np.array_equal(R.decode(snap.header.download((history.header_bytes(vol.n),), np.uint8),
                                       snap.pool.download((max(64 * snap.literal_blocks, 16),), np.uint8), vol.n), first.reshape(-1))
        tris_before = vol.marching_cubes(download=True).copy()
        vol.region_grow([seed], 226, 3071, _structure(3, 1))
        grown = vol.download_mask().copy()
        assert not np.array_equal(grown, first)
        grown_snap = vol.snapshot_mask()
        vol.restore_mask(snap)
        assert np.array_equal(vol.download_mask(), first)
        assert np.array_equal(vol.marching_cubes(download=True), tris_before)  # planes, levels and counts were dropped
        vol.restore_mask(grown_snap)
        assert np.array_equal(vol.download_mask(), grown)
        snap.close()
        grown_snap.close()
        with pytest.raises(ValueError):
            vol.restore_mask(snap)
    assert history.live_device_blocks() == live


def test_undo_after_a_region_growth_at_129_cubed(ivxlib):
    from invesalius3_amd import history, resident, styles
    from invesalius3_amd import mask as mk
    image = synth_volume((129, 129, 129))
    m = np.zeros((130, 130, 130), np.uint8)
    m[1:, 1:, 1:] = np.where(image >= 226, 255, 0)
    m[1:, 0, 0] = 1
    saved = m.copy()
    z, y, x = (int(v) for v in np.unravel_index(int(np.argmax(image)), image.shape))
    with mk.bind_matrix(m):
        h = history.EditionHistory()
        with history.recorded(h, m) as rec:
            rec.result = styles.do_3d_seg(image, m, (x, y, z), method="threshold", con_3d=26, t0=226, t1=3071)
        assert rec.result is True and (m == 254).any()
        grown = m.copy()
        s = resident.transfer_stats()
        h.undo(m, None)
        up, down = _moved(s)
        assert np.array_equal(m, saved)
        changed = int((grown != saved).any(axis=(1, 2)).sum())
        assert up == 0 and down == changed * 130 * 130
        h.redo(m, None)
        assert np.array_equal(m, grown)
        resident.set_check(True)
        try:
            history.snapshot(m).close()
        finally:
            resident.set_check(False)
        h.clear_history()
