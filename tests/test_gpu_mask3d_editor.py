"""GPU: the 3-D mask editor (csrc/k_mask3d.hip, invesalius3_amd/mask3d_editor.py) against the existing invesalius_rs calls
it replaces -- polygon2mask_rs, mask_cut, brush_mask_rs on contiguous copies -- byte for byte over the whole padded matrix."""
import ctypes
import json
import os

import numpy as np
import pytest

import _mask3d_ref as R
from invesalius3_amd import _lib as L
from invesalius3_amd import history as H
from invesalius3_amd import invesalius_rs as rs
from invesalius3_amd import mask as mask_mod
from invesalius3_amd import mask3d_editor as M3
from invesalius3_amd import resident
from invesalius3_amd.device import DeviceBuffer
from test_mask3d_editor_host import POLYGONS, brush_cases, filter_sets

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SPACING = (0.5, 0.75, 1.25)
CUT_SHAPES = [(1, 1, 1), (4, 6, 15), (3, 5, 16), (5, 7, 19), (2, 9, 32), (3, 17, 33)]


# ---- filter ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(37, 23), (1, 1), (64, 48)])
@pytest.mark.parametrize("mode", [0, 1])
def test_filter_equals_the_composition_of_polygon2mask_rs(ivxlib, size, mode):
    w, h = size
    some = 0
    for names in filter_sets():
        polys = [np.asarray(POLYGONS[n], np.float64).reshape(-1, 2) for n in names]
        want = R.np_filter(size, polys, mode, rs.polygon2mask_rs)
        got = M3.polygon_filter(size, polys, mode)
        assert got.shape == (h, w) and got.dtype == np.bool_
        assert np.array_equal(got, want), names
        some += int(want.sum())
    assert some


def test_filter_has_no_point_cap(ivxlib):
    """the points are read from global memory: a polygon of 5000 points goes the same way as one of 3"""
    t = np.linspace(0.0, 2.0 * np.pi, 5000, endpoint=False)
    poly = np.stack([30.0 + 25.0 * np.cos(t) * (1.0 + 0.2 * np.sin(7 * t)), 22.0 + 18.0 * np.sin(t)], axis=1)
    for mode in (0, 1):
        assert np.array_equal(M3.polygon_filter((64, 48), [poly, POLYGONS["triangle"]], mode),
                              R.np_filter((64, 48), [poly, POLYGONS["triangle"]], mode, rs.polygon2mask_rs))


# ---- cut ------------------------------------------------------------------------------------------------------------------------
def cut_matrices(shape, fsize):
    """(name, m, mv, depth): orthographic from outside, a pinhole inside (voxels behind the eye), an exact pixel grid whose last
    columns leave the screen; each with a depth that cuts through the volume"""
    (om, omv), cam = R.ortho_matrices(shape, SPACING, fsize)
    near, far = M3.default_clipping_range(cam)
    yield "orthographic", om, omv, near + (far - near) * 0.5
    pm, pmv = R.perspective_matrices(shape, SPACING)
    yield "perspective", pm, pmv, 0.55 * float(np.linalg.norm([(s - 1) * sp for s, sp in zip(shape[::-1], SPACING)])) + 0.3
    m, mv = R.pixel_matrices(shape, SPACING, fsize, step=(0.45, 0.8))
    yield "pixel grid", m, mv, 0.7 * float(np.linalg.norm([(s - 1) * sp for s, sp in zip(shape[::-1], SPACING)])) + 0.2


def rs_cut(matrix, fsize_filter, m, mv, depth, mode):
    """the parent's way: mask_cut on a contiguous copy of the interior, written back"""
    want = matrix.copy()
    interior = np.ascontiguousarray(want[1:, 1:, 1:])
    rs.mask_cut(interior.copy(), SPACING[0], SPACING[1], SPACING[2], depth, fsize_filter, m, mv, interior, mode)
    want[1:, 1:, 1:] = interior
    return want


def dev_cut(matrix, filt, m, mv, depth, mode, offset):
    """ivx_dev_m3e_cut on a device copy that starts `offset` bytes past an aligned address -> (matrix after, plane flags)"""
    n = matrix.nbytes
    blk, d_f, d_flags = DeviceBuffer(n + 64), DeviceBuffer(max(filt.size, 16)), DeviceBuffer(matrix.shape[0] + 16)
    try:
        blk.zero()
        d_flags.zero()
        L.check(L.lib().ivx_memcpy_h2d(blk.at(offset), L.ptr(matrix), n))
        d_f.upload(np.ascontiguousarray(filt).view(np.uint8))
        m, mv = np.ascontiguousarray(m, np.float64), np.ascontiguousarray(mv, np.float64)
        L.check(L.lib().ivx_dev_m3e_cut(blk.at(offset), L.i64([s - 1 for s in matrix.shape]), L.i64(matrix.strides), M3._d3(SPACING),
                                        float(depth), d_f.ptr, filt.shape[0], filt.shape[1], L.ptr(m), L.ptr(mv), mode, d_flags.ptr, None),
                "dev cut")
        L.synchronize()
        whole = blk.download((n + 64,), np.uint8)
        assert not whole[:offset].any() and not whole[offset + n:].any()  # nothing outside the matrix
        return whole[offset:offset + n].reshape(matrix.shape).copy(), d_flags.download((matrix.shape[0],), np.uint8)
    finally:
        for b in (blk, d_f, d_flags):
            b.close()


@pytest.mark.parametrize("shape", CUT_SHAPES)
@pytest.mark.parametrize("mode", [0, 1])
def test_cut_equals_mask_cut_on_every_alignment(ivxlib, shape, mode):
    fsize = (13, 9)
    filt = R.random_filter(fsize)
    changed_any = kept_any = 0
    for k, (name, m, mv, depth) in enumerate(cut_matrices(shape, fsize)):
        for fill in (None, 0, 255):
            matrix = R.padded(R.volume(shape, 40 + k, fill))
            want = rs_cut(matrix, filt, m, mv, depth, mode)
            for offset in (0, 1, 7) if fill is None else (0,):
                got, flags = dev_cut(matrix, filt, m, mv, depth, mode, offset)
                assert np.array_equal(got, want), (name, fill, offset)
                assert np.array_equal(flags.astype(bool), (matrix != got).any(axis=(1, 2))), (name, fill, offset)
            changed_any += int((want != matrix).sum())
            kept_any += int((want[1:, 1:, 1:] > 127).sum())
    if shape != (1, 1, 1):
        assert changed_any and kept_any


@pytest.mark.parametrize("bound", [False, True])
def test_cut_host_form_filter_or_polygons(ivxlib, bound):
    shape, size = (5, 7, 19), (37, 23)
    (m, mv), cam = R.ortho_matrices(shape, SPACING, size)
    near, far = M3.default_clipping_range(cam)
    polys = [POLYGONS["triangle"], POLYGONS["concave"]]
    for mode in (0, 1):
        filt = R.np_filter(size, polys, mode, rs.polygon2mask_rs)
        start = R.padded(R.volume(shape, 50))
        want = rs_cut(start, filt, m, mv, far, mode)
        assert (want != start).any()
        for arg in (filt, polys):
            matrix = start.copy()
            res = mask_mod.bind_matrix(matrix) if bound else None
            resident.set_check(True)
            try:
                written = M3.cut_mask(matrix, SPACING, arg, size, m, mv, far, mode)
                assert np.array_equal(matrix, want)
                assert written == int((want != start).any(axis=(1, 2)).sum())
                if bound:  # host and mirror hold the same bytes: the next use passes the stale check and reads the cut state
                    assert M3.cut_mask(matrix, SPACING, arg, size, m, mv, far, mode) == 0
                    assert np.array_equal(matrix, want)
            finally:
                resident.set_check(False)
                if res is not None:
                    res.release()


# ---- brush ----------------------------------------------------------------------------------------------------------------------
def rs_stroke(matrix, orig, centres, radius, mode):
    want = matrix.copy()
    interior = np.ascontiguousarray(want[1:, 1:, 1:])
    o = np.ascontiguousarray(orig[1:, 1:, 1:]) if orig is not None else None
    for c in centres:
        rs.brush_mask_rs(interior, o, SPACING, tuple(float(v) for v in c), radius, mode)
    want[1:, 1:, 1:] = interior
    return want


def world_of(centres):
    """the world points whose reference arithmetic (wx + sx, -wy - sy, wz + sz) gives these centres"""
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    w = np.stack([c[:, 0] - SPACING[0], -(c[:, 1] + SPACING[1]), c[:, 2] - SPACING[2]], axis=1)
    assert np.array_equal(M3.brush_centres(w, SPACING), c)  # (the cases below are exact in binary)
    return w


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("with_orig", [False, True])
def test_one_dab_equals_brush_mask_rs(ivxlib, mode, with_orig):
    shape = (5, 7, 19)
    start = R.padded(R.volume(shape, 61))
    orig = R.padded(R.volume(shape, 62)) if with_orig else None
    changed = 0
    for name, c, radius in brush_cases():
        c = tuple(np.round(np.asarray(c) * 64) / 64)  # binary fractions: world_of is exact
        matrix = start.copy()
        want = rs_stroke(start, orig, [c], radius, mode)
        written = M3.brush_stroke(matrix, orig, SPACING, world_of([c]), 2.0 * radius, mode)
        assert np.array_equal(matrix, want), name
        assert written == int((want != start).any(axis=(1, 2)).sum()), name
        changed += int((want != start).sum())
    assert (changed > 0) == (mode in (0, 1))


def stroke_centres(n, shape, seed):
    """n centres on a 1/64 grid along a path through the volume and out of it, neighbours overlapping"""
    rng = np.random.default_rng(seed)
    d, h, w = shape
    t = np.linspace(-0.15, 1.15, n) if n > 2 else np.linspace(0.35, 0.6, n)  # (one or two dabs: inside, overlapping)
    c = np.stack([t * (w - 1) * SPACING[0], (0.5 + 0.4 * np.sin(5 * t)) * (h - 1) * SPACING[1], (1 - t) * (d - 1) * SPACING[2]], axis=1)
    c += rng.normal(0, 0.2, c.shape)
    return np.round(c * 64) / 64


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("with_orig", [False, True])
def test_stroke_equals_the_dabs_one_after_another(ivxlib, mode, with_orig):
    cap = M3.brush_capacity()
    shape = (6, 9, 21)
    start = R.padded(R.volume(shape, 71))
    orig = R.padded(R.volume(shape, 72)) if with_orig else None
    for n, radius in ((1, 1.6), (2, 1.6), (7, 1.6), (cap, 0.8), (cap + 1, 0.8)):
        centres = stroke_centres(n, shape, 73 + n)
        want = rs_stroke(start, orig, centres, radius, mode)
        assert (want != start).any()
        for bound in (False, True):
            matrix = start.copy()
            res = mask_mod.bind_matrix(matrix) if bound else None
            try:
                written = M3.brush_stroke(matrix, orig, SPACING, world_of(centres), 2.0 * radius, mode)
                assert np.array_equal(matrix, want), (n, bound)
                assert written == int((want != start).any(axis=(1, 2)).sum()), (n, bound)
            finally:
                if res is not None:
                    res.release()


def test_stroke_split_at_the_capacity_reaches_the_last_dab(ivxlib):
    """dab capacity + 1 goes into a second launch: put it where no other dab reaches"""
    cap = M3.brush_capacity()
    shape = (6, 9, 21)
    start = R.padded(R.volume(shape, 0, 255))
    centres = np.tile(np.array([[1.0, 1.5, 1.25]]), (cap + 1, 1))
    centres[cap] = [9.0, 4.5, 5.0]
    matrix = start.copy()
    M3.brush_stroke(matrix, None, SPACING, world_of(centres), 1.0, 1)
    assert np.array_equal(matrix, rs_stroke(start, None, centres, 0.5, 1))
    assert matrix[1 + 4, 1 + 6, 1 + 18] == 0  # (x, y, z) = (18, 6, 4) = the last centre / spacing


# ---- equal ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4099, 70001])
def test_equal(ivxlib, n):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, n + 3).astype(np.uint8)
    da, db = DeviceBuffer(n + 16), DeviceBuffer(n + 16)
    try:
        for off_a, off_b in ((0, 0), (1, 0), (3, 3)):
            for at in (None, 0, n // 2, n - 1):
                b = a[off_a:off_a + n].copy()
                if at is not None:
                    b[at] ^= 1
                L.check(L.lib().ivx_memcpy_h2d(da.at(off_a), L.ptr(np.ascontiguousarray(a[off_a:off_a + n])), n))
                L.check(L.lib().ivx_memcpy_h2d(db.at(off_b), L.ptr(b), n))
                eq = ctypes.c_int(-1)
                L.check(L.lib().ivx_dev_m3e_equal(da.at(off_a), db.at(off_b), n, ctypes.byref(eq), None))
                assert eq.value == int(at is None), (off_a, off_b, at)
    finally:
        da.close()
        db.close()


# ---- the state machine ------------------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self, state_ref):
        self.sent, self.state_ref = [], state_ref

    def __call__(self, topic, **kw):
        self.sent.append(topic)
        st = self.state_ref[0]
        # the viewer answers at once, like the reference's
        if topic == "Send volume viewer size":
            st.ReceiveVolumeViewerSize(self.size)
        elif topic == "Send volume viewer active camera" and self.size[1] != 0:  # (the fixture's viewer: see its notes)
            st.ReceiveVolumeViewerActiveCamera(self.camera)


def golden():
    path = os.path.join(HERE, "golden", "ref_mask3deditor.npz")
    return np.load(path, allow_pickle=False)


def replay(G, script, bound):
    """run one script of the fixture; compare after every call"""
    steps = script["steps"]
    spacing = tuple(script["spacing"])
    start = G[script["matrix"]].copy() if script["matrix"] else None
    matrix = start.copy() if start is not None else None
    res = mask_mod.bind_matrix(matrix) if (bound and matrix is not None) else None
    ref = [None]
    rec = Recorder(ref)
    rec.size = tuple(script["size"])
    rec.camera = (G[script["m"]], G[script["mv"]], tuple(script["clipping_range"]))
    hist = H.EditionHistory(publish=rec)
    st = ref[0] = M3.Mask3DEditorState(matrix, spacing, rec.size, publish=rec, history=hist, mask_3d_preview=script["mask_3d_preview"])
    # the fixture's vtkCoordinate stand-in, as the table of what it answered: the very doubles the reference rasterised
    table = {tuple(r[:3]): tuple(r[3:]) for r in script["display_table"]}
    st.to_display = lambda world_points: np.array([table[tuple(float(v) for v in p)] for p in world_points], np.float64).reshape(-1, 2)
    resident.set_check(True)
    try:
        for i, step in enumerate(steps):
            rec.sent.clear()
            name, args = step["call"], step.get("args", [])
            if name == "set_size":
                rec.size = tuple(args)
                continue
            if name == "host_edit":  # another tool writes the mask between two uses of the editor
                matrix[2:4, 2:5, 3:8] = 255
                resident.touch(matrix[2:4])
                continue
            if name == "host_restore":
                matrix[...] = start
                resident.touch(matrix)
                continue
            getattr(st, name)(*args)
            where = (script["name"], i, name)
            sent = [t for t in rec.sent if t not in ("Enable undo", "Enable redo")]
            assert sent == step["sent"], where
            if matrix is not None:
                assert np.array_equal(matrix, G[step["matrix"]]), where
            if step["mask_data"]:
                assert np.array_equal(st.download("mask_data"), G[step["mask_data"]]), where
            else:
                assert st.mask_data is None, where
            assert st.has_cleared_for_crop == step["has_cleared_for_crop"], where
        assert len(hist.history) == 2 * script["history_nodes"], script["name"]
        if matrix is not None and bound:  # host and mirror agree at the end
            snap = H.snapshot(matrix)
            check = np.zeros_like(matrix)
            H.restore(snap, check)
            snap.close()
            assert np.array_equal(check, matrix), script["name"]
    finally:
        resident.set_check(False)
        st.close()
        hist.clear_history()
        if res is not None:
            res.release()


@pytest.mark.parametrize("bound", [False, True])
def test_state_machine_replays_the_references_scripts(ivxlib, bound):
    G = golden()
    scripts = json.loads(str(G["scripts"]))
    assert len(scripts) >= 6
    for script in scripts:
        replay(G, script, bound)


# ---- link traffic -----------------------------------------------------------------------------------------------------------------
def test_link_traffic_on_a_bound_matrix(ivxlib):
    shape, size = (12, 20, 33), (64, 48)
    matrix = R.padded(R.volume(shape, 81, 255), guard=False)
    plane = matrix[0].nbytes
    (m, mv), cam = R.ortho_matrices(shape, SPACING, size)
    cam = dict(cam, clipping_range=M3.default_clipping_range(cam))
    res = mask_mod.bind_matrix(matrix)
    hist = H.EditionHistory()
    st = M3.Mask3DEditorState(matrix, SPACING, size, history=hist)
    try:
        st.setup_state()
        st.ReceiveVolumeViewerActiveCamera(cam)
        centre = np.array([16 * SPACING[0], -10 * SPACING[1], 6 * SPACING[2]])  # world: y is negated
        corners = centre + np.array([[-3.0, 0, -2.0], [3.0, 0.5, -2.0], [0.0, -0.5, 3.0]])
        for (x, y), wp in zip(M3.world_to_display(corners, cam, size), corners):
            st.insert_point(x, y, tuple(wp))

        def moved(fn):
            before, m0 = resident.transfer_stats(), matrix.copy()
            fn()
            after = resident.transfer_stats()
            changed = int((m0 != matrix).any(axis=(1, 2)).sum())
            return after["h2d_bytes"] - before["h2d_bytes"], after["d2h_bytes"] - before["d2h_bytes"], changed

        up, down, changed = moved(st.complete_current_polygon)  # a cut
        assert changed > 0 and up <= 256 and down == changed * plane, (up, down, changed)  # up: the polygon's points
        # the next preview picture reads the cut state from the mirror: it moves its tables and its picture, no mask byte
        from invesalius3_amd import volume_mask
        served = resident.transfer_stats()["served_bytes"]
        up1, down1, _ = moved(lambda: volume_mask.mask_preview(matrix, SPACING, (0.0, 1.0, 0.0), cam, size, rgba8=True))
        assert resident.transfer_stats()["served_bytes"] - served >= matrix.nbytes
        up2, down2, _ = moved(lambda: volume_mask.mask_preview(matrix, SPACING, (0.0, 1.0, 0.0), cam, size, rgba8=True))
        assert (up1, down1) == (up2, down2) and up1 < matrix.nbytes and down1 == size[0] * size[1] * 4, (up1, down1, up2, down2)
        up, down, changed = moved(lambda: st.SetDepthValue(0.5))  # a depth tick (cumulative: nothing more to cut is possible)
        assert up <= 256 and down == changed * plane, (up, down, changed)
        st.SetToolMode(M3.MASK_3D_EDIT_TOOL_BRUSH)
        st.SetBrushSize(4.0)
        up, down, _ = moved(st.start_brush_stroke)
        assert (up, down) == (0, 0)
        dabs = np.array([[2.0 + 0.7 * k, -3.0 - 0.4 * k, 2.0 + 0.5 * k] for k in range(7)])
        up, down, changed = moved(lambda: st.brush_stroke(dabs))
        assert changed > 0 and up == dabs.nbytes and down == changed * plane, (up, down, changed)  # up: the centres
        up, down, _ = moved(st.end_brush_stroke)
        assert (up, down) == (0, 0)
        assert (matrix[0] == 1).all() and (matrix[:, 0, :] == 1).all() and (matrix[:, :, 0] == 1).all()
        assert hist.index == 1
        # host and mirror agree: a snapshot of the bound matrix (read from the mirror) decodes to the host's bytes
        resident.set_check(True)
        snap = H.snapshot(matrix)
        check = np.zeros_like(matrix)
        H.restore(snap, check)
        snap.close()
        assert np.array_equal(check, matrix)
    finally:
        resident.set_check(False)
        st.close()
        hist.clear_history()
        res.release()
