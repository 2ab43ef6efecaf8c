"""GPU: the slice editing tools -- brush strokes, the lazy per-slice threshold, the buffer write-back, the fill
brushes, 2-D region growing and crop mask -- against the reference's own output (tests/golden/ref_editor.npz) and, where the
fixture has no case, the numpy restatement that tests/test_editor_host.py holds against it.  Every mask is compared over the
WHOLE padded matrix: nothing outside the slice may change, and the flags must be right.

Shapes: an image of (9, 20, 24) with its (10, 21, 25) padded mask -- odd pitches, so the coronal and sagittal views are
unaligned -- start values from {0, 1, 2, 253, 254, 255}, flags mixed across 0, 1 and 2; an 81 x 81 disk on (3, 100, 120) has more
pixels than one workgroup has threads; a radius-30 disk is larger than every slice of the small volume."""
import gc
import json

import numpy as np
import pytest

import _editor_cases as C
import _editor_ref as R

pytestmark = pytest.mark.gpu
G = C.golden
POSITIONS = [(3, 3), (2, 2), (1, 5), (0, 0), (-4, 5), (-5, 5), (-8, 5), (23, 10), (30, 10), (10, -9), (22, 10), (5.5, 5.5),
             (10, 0), (10, 1000), (0, 4), (1000, 4), (-1000, -1000), (7.99, 3.01), (-0.5, -0.5), (23, 19), (0, 8), (19, 0), 45, 0, 170, 10 ** 6]


def _ranges():
    g = G()
    return tuple(float(v) for v in g["edition_range"]), tuple(int(v) for v in g["threshold_range"])


@pytest.fixture(autouse=True)
def _registry_returns_to_what_it_was(ivxlib):
    from invesalius3_amd import resident
    before = resident.count()
    yield
    resident.set_check(False)
    gc.collect()
    assert resident.count() == before


# ---- one dab -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vol", ["small", "big"])
def test_every_recorded_dab_equals_the_reference(ivxlib, vol):
    """every operation x orientation x footprint x position of the fixture: the slice is the reference's buffer slice after
    Slice.edit_mask_pixel, its flag is 2, and no other byte of the padded matrix moved"""
    from invesalius3_amd import slice_
    edition, _ = _ranges()
    image, padded = C.volume(vol)
    seen = set()
    for ori, n, op, fp, pos, want in C.dab_cases(vol):
        m = padded.copy()
        m[R.flag_index(ori, n)] = 1  # the reference's dab acts on the buffer slice as it stands: no lazy threshold in front
        prev = slice_.edit_mask_pixel(m, image, ori, n, op, C.footprint(fp), pos, edition, return_previous=True)
        ref = padded.copy()
        C.slice_of(ref[1:, 1:, 1:], ori, n)[...] = want
        ref[R.flag_index(ori, n)] = 2
        assert np.array_equal(m, ref), (ori, n, op, fp, pos)
        assert np.array_equal(prev, C.slice_of(padded[1:, 1:, 1:], ori, n))
        seen.add((ori, op, fp))
    assert len(seen) == (3 * (6 + 9) if vol == "small" else 9)


@pytest.mark.parametrize("orientation,n", [("AXIAL", 2), ("AXIAL", 0), ("CORONAL", 19), ("SAGITAL", 23)])  # flags 0, 1, 2, 0
def test_every_operation_footprint_and_position_with_the_lazy_threshold(ivxlib, orientation, n):
    """the whole flow of one brush event -- get_mask_slice (acts on flag 0 only), the dab, the write-back with flag 2 -- against
    the restatement, for six operations x five footprints x the position list (edges, corners, misses, floats, flat integers)"""
    from invesalius3_amd import cursor, slice_
    edition, thr = _ranges()
    g = G()
    image, padded = C.volume("small")
    prints = [C.footprint(0), cursor.cursor_pixels("rectangle", 4.2, "mm", tuple(g["spacing"]), orientation), C.footprint(3), C.footprint(1),
              cursor.cursor_pixels("rectangle", 0.2, "mm", tuple(g["spacing"]), "CORONAL")]
    assert prints[1].size > 0 and prints[4].size == 0  # an empty rectangle paints nothing and is no error
    for op in range(6):
        for k, index in enumerate(prints):
            for pos in (POSITIONS if k < 3 else POSITIONS[:4] + POSITIONS[-4:]):
                m, ref = padded.copy(), padded.copy()
                slice_.edit_mask_pixel(m, image, orientation, n, op, index, pos, edition, threshold_range=thr)
                R.stroke(ref, image, orientation, n, index, [pos], op, edition, thr)
                assert np.array_equal(m, ref), (op, index.shape, pos)


# ---- strokes -------------------------------------------------------------------------------------------------------------------------
def _strokes(w, h):
    diagonal = [(k * 1.3 - 5, k * 0.9 - 4) for k in range(40)]                      # 40 dabs on a diagonal that leaves the slice
    there_and_back = [(k, 4) for k in range(2, w - 2)] + [(k, 5) for k in range(w - 3, 1, -1)]  # returns over itself
    mixed = [(k, h // 2) for k in range(w)]
    mixed_ops = [0] * 10 + [5] * (w - 16) + [1] * 6   # DRAW, then THRESH_ERASE_ONLY, then ERASE: later runs overwrite earlier ones
    return [("diagonal", diagonal, 2), ("diagonal draw", diagonal, 0), ("there and back", there_and_back, 3),
            ("mixed", mixed + mixed[::-1], mixed_ops + mixed_ops[::-1])]


@pytest.mark.parametrize("orientation,n", [("AXIAL", 5), ("CORONAL", 6), ("SAGITAL", 23)])
def test_strokes_equal_the_dabs_one_after_another(ivxlib, orientation, n):
    from invesalius3_amd import slice_
    edition, thr = _ranges()
    image, padded = C.volume("small")
    h, w = C.slice_of(image, orientation, n).shape
    for name, positions, ops in _strokes(w, h):
        for index in (C.footprint(0), C.footprint(2)):
            m, ref = padded.copy(), padded.copy()
            prev = slice_.edit_mask_stroke(m, image, orientation, n, index, positions, ops, edition, threshold_range=thr, return_previous=True)
            p_ref = R.stroke(ref, image, orientation, n, index, positions, ops, edition, thr)
            assert np.array_equal(m, ref), (name, index.shape)
            assert np.array_equal(prev, p_ref), name
            again = padded.copy()
            slice_.edit_mask_stroke(again, image, orientation, n, index, positions, ops, edition, threshold_range=thr)
            assert np.array_equal(again, m), name        # the same bytes on a second run
            slice_.edit_mask_stroke(again, image, orientation, n, index, positions, ops, edition, threshold_range=thr)
            assert np.array_equal(again, m), name        # and the stroke over its own result changes nothing


def test_big_footprint_stroke_on_the_big_volume(ivxlib):
    """81 x 81 pixels per dab (26 workgroups each), 30 dabs that cross the slice and leave it"""
    from invesalius3_amd import slice_
    edition, thr = _ranges()
    image, padded = C.volume("big")
    positions = [(k * 5 - 20, k * 3.5 - 10) for k in range(30)]
    for ori, n in (("AXIAL", 1), ("CORONAL", 50), ("SAGITAL", 119)):
        for ops in (2, [4] * 10 + [1] * 10 + [3] * 10):
            m, ref = padded.copy(), padded.copy()
            slice_.edit_mask_stroke(m, image, ori, n, C.footprint(4), positions, ops, edition, threshold_range=thr)
            R.stroke(ref, image, ori, n, C.footprint(4), positions, ops, edition, thr)
            assert np.array_equal(m, ref), (ori, ops)


# ---- bound and unbound, and what crosses the link ---------------------------------------------------------------------------------------
def _xfer():
    from invesalius3_amd import resident
    s = resident.transfer_stats()
    return s["h2d_bytes"], s["d2h_bytes"]


def test_bound_matrices_same_bytes_and_the_stroke_moves_one_slice(ivxlib):
    from invesalius3_amd import mask as mk
    from invesalius3_amd import resident, slice_
    edition, thr = _ranges()
    image, padded = C.volume("small")
    image = image.copy()
    index = C.footprint(0)
    positions = [(k * 0.7, k * 0.4 + 1) for k in range(25)]
    n = 11
    for ori in C.ORIENTATIONS:
        for ops in (2, 0, [5] * 12 + [3] * 13):
            ref = padded.copy()
            slice_.edit_mask_stroke(ref, image.copy(), ori, 3, index, positions, ops, edition, threshold_range=thr)  # unbound
            want = padded.copy()
            R.stroke(want, image, ori, 3, index, positions, ops, edition, thr)
            assert np.array_equal(ref, want)
            m = padded.copy()
            with slice_.bind_image(image), mk.bind_matrix(m):
                resident.set_check(True)   # every use compares host and mirror first: raises on a mirror that fell behind
                slice_.edit_mask_stroke(m, image, ori, 3, index, positions, ops, edition, threshold_range=thr)
                slice_.get_mask_slice(m, image, ori, 3, thr)
                slice_.do_threshold_to_all_slices(m, image, thr)
                resident.set_check(False)
            R.do_threshold_to_all_slices(want, image, thr)
            assert np.array_equal(m, want), (ori, ops)
    # the counters, check off: a sagittal stroke moves no image or mask byte host -> device -- the footprint and the dab list
    # are all that goes up -- and at most one slice plus the flag device -> host
    m = padded.copy()
    h, w = image.shape[0], image.shape[1]
    with slice_.bind_image(image), mk.bind_matrix(m) as rm:
        slice_.get_mask_slice(m, image, "SAGITAL", n, thr)
        up0, down0 = _xfer()
        slice_.edit_mask_stroke(m, image, "SAGITAL", n, index, positions, 2, edition)
        up1, down1 = _xfer()
        assert up1 - up0 == index.size + 8 * len(positions), up1 - up0
        assert 0 < down1 - down0 <= h * w + 1, down1 - down0
        want = padded.copy()
        R.stroke(want, image, "SAGITAL", n, index, positions, 2, edition, thr)
        assert np.array_equal(m, want) and m[0, 0, n + 1] == 2
        # what follows sees the edit without an upload: the lazy threshold of the (flagged) slice, a MaxIP of the mask, and the
        # threshold of the stale slices (which sends up the flag cells it wrote, one byte per slice, and nothing else)
        up0, _ = _xfer()
        got = slice_.get_mask_slice(m, image, "SAGITAL", n, thr)
        mip = slice_.project(m[1:, 1:, 1:], 2, slice_.PROJECTION_MaxIP)
        assert _xfer()[0] == up0
        assert np.array_equal(got, want[1:, 1:, n + 1]) and np.array_equal(mip, want[1:, 1:, 1:].max(axis=2))
        slice_.do_threshold_to_all_slices(m, image, thr)
        assert _xfer()[0] - up0 == image.shape[0]
        R.do_threshold_to_all_slices(want, image, thr)
        assert np.array_equal(m, want)
        resident.set_check(True)
        slice_.project(m[1:, 1:, 1:], 0, slice_.PROJECTION_MaxIP)  # host and mirror agree byte for byte
        assert rm.stats()["refresh_bytes"] == 0  # nothing was ever touched: the library wrote host and mirror itself


# ---- the tools -------------------------------------------------------------------------------------------------------------------------
def test_get_mask_slice_and_apply_slice_buffer(ivxlib):
    from invesalius3_amd import mask as mk
    from invesalius3_amd import resident, slice_
    g = G()
    _, thr = _ranges()
    for (o, n), want in zip(g["getslice_meta"], g["getslice_out"]):
        ori = C.ORIENTATIONS[o]
        m = g["mask_in"].copy()
        got = slice_.get_mask_slice(m, g["img"], ori, int(n), thr)
        assert np.array_equal(m, want) and np.array_equal(got, g["getslice_ret_%s_%d" % (ori, n)]), (ori, n)
        if g["mask_in"][R.flag_index(ori, int(n))] != 0:
            assert np.array_equal(m, g["mask_in"])  # a flagged slice: nothing happens
        got[...] = 7
        assert np.array_equal(m, want)  # a copy, not a view
    for bound in (False, True):
        for ori, want in zip(C.ORIENTATIONS, g["apply_out"]):
            m = g["mask_in"].copy()
            if bound:
                with mk.bind_matrix(m):
                    prev = slice_.apply_slice_buffer_to_mask(m, ori, 5, g["apply_b_%s" % ori])
                    resident.set_check(True)
                    slice_.project(m, 0, slice_.PROJECTION_MaxIP)  # the mirror got the slice and the flag
                    resident.set_check(False)
            else:
                prev = slice_.apply_slice_buffer_to_mask(m, ori, 5, g["apply_b_%s" % ori])
            assert np.array_equal(m, want) and np.array_equal(prev, g["apply_prev_%s" % ori]), (ori, bound)


def test_brush_fill_on_an_unpadded_marker_matrix(ivxlib):
    from invesalius3_amd import styles
    g = G()
    for row, want in zip(g["fill_meta"], g["fill_out"]):
        ori, n, value, fp = C.ORIENTATIONS[int(row[0])], int(row[1]), int(row[2]), int(row[3])
        m = g["markers_in"].copy()
        styles.brush_fill(m, ori, n, value, C.footprint(fp), C.position(row[4:7]))
        assert np.array_equal(m, want), row
    # a drag in one call
    m, ref = g["markers_in"].copy(), g["markers_in"].copy()
    positions = [(k, k * 0.5) for k in range(-3, 30)]
    styles.brush_fill(m, "CORONAL", 19, 2, C.footprint(0), positions=positions)
    for p in positions:
        R.fill_pixel(ref[:, 19, :], 2, C.footprint(0), p)
    assert np.array_equal(m, ref)


def test_do_2d_seg_equals_the_reference(ivxlib):
    from invesalius3_amd import styles
    g = G()
    ww, wl = (int(v) for v in g["seg2d_wwwl"])
    kinds = set()
    for row, want in zip(g["seg2d_meta"], g["seg2d_out"]):
        method, use, con, ax, n, x, y, t0, t1, dmin, dmax = (int(v) for v in row)
        m = g["mask_in"].copy()
        got = styles.do_2d_seg(g["img"], m, (x, y), C.ORIENTATIONS[ax], n, C.METHODS[method], con, 254, t0, t1, dmin, dmax, bool(use), ww, wl,
                               2.5, 3)
        assert np.array_equal(m, want), row   # the whole matrix: no flag touched (the reference's quirk), nothing outside the slice
        if np.array_equal(want, g["mask_in"]):
            assert got is False               # the rejected click
        else:
            assert np.array_equal(got, C.slice_of(g["mask_in"][1:, 1:, 1:], C.ORIENTATIONS[ax], n))
        kinds.add((method, use, con, ax))
    assert len(kinds) == 9 and {k[3] for k in kinds} == {0, 1, 2} and {k[2] for k in kinds} == {4, 8}


def test_crop_mask(ivxlib):
    from invesalius3_amd import mask as mk
    from invesalius3_amd import resident, slice_, styles
    g = G()
    _, thr = _ranges()
    for box, want in zip(g["crop_boxes"], g["crop_out"]):  # a box on a face, one voxel, the whole volume, a corner
        m = g["mask_in"].copy()
        styles.crop_mask(m, g["img"], tuple(int(v) for v in box), thr)
        assert np.array_equal(m, want), box
        m = g["mask_in"].copy()
        with slice_.bind_image(g["img"].copy()) as ri, mk.bind_matrix(m):
            styles.crop_mask(m, ri.array, tuple(int(v) for v in box), thr)
            resident.set_check(True)
            slice_.project(m, 0, slice_.PROJECTION_MaxIP)
            resident.set_check(False)
        assert np.array_equal(m, want), box
    # a volume whose padded size is no multiple of the 16-byte chunks, and a box that reaches past it
    image, padded = C.volume("big")
    m, ref = padded.copy(), padded.copy()
    styles.crop_mask(m, image, (17, 500, 3, 51, 1, 1), thr)
    R.crop_mask(ref, image, (17, 500, 3, 51, 1, 1), thr)
    assert np.array_equal(m, ref)
    with pytest.raises(ValueError):
        styles.crop_mask(m, image, (-1, 5, 0, 5, 0, 1), thr)


def test_device_volume_forms_equal_the_host_forms(ivxlib):
    from invesalius3_amd import slice_, styles
    from invesalius3_amd.device import DeviceBuffer, DeviceVolume
    edition, thr = _ranges()
    g = G()
    image, padded = C.volume("small")
    positions = [(k * 1.1 - 3, k * 0.6) for k in range(30)]
    ops = [0] * 8 + [4] * 8 + [5] * 8 + [1] * 6
    with DeviceVolume(image) as vol:
        for ori, n in (("AXIAL", 0), ("CORONAL", 19), ("SAGITAL", 23)):
            for index in (C.footprint(0), C.footprint(3)):
                host = padded.copy()
                host[R.flag_index(ori, n)] = 1  # (up to date: the device form has no flags and no lazy threshold)
                slice_.edit_mask_stroke(host, image, ori, n, index, positions, ops, edition)
                vol.mask.upload_view(padded[1:, 1:, 1:])
                vol.brush_stroke(ori, n, index, positions, ops, edition)
                assert np.array_equal(vol.download_mask(), host[1:, 1:, 1:]), (ori, index.shape)
        # the fill brush on a marker block
        markers = DeviceBuffer(image.size)
        host = g["markers_in"].copy()
        markers.upload(host)
        styles.brush_fill(host, "SAGITAL", 22, 2, C.footprint(0), positions=positions)
        vol.brush_fill("SAGITAL", 22, 2, C.footprint(0), positions, target=markers)
        assert np.array_equal(markers.download(image.shape, np.uint8), host)
        markers.close()
        # crop: the resident mask is the interior of the padded matrix
        for box in g["crop_boxes"]:
            host = padded.copy()
            host[1:, 0, 0] = 1  # (every slice up to date: the device form has no flags to look at)
            styles.crop_mask(host, image, tuple(int(v) for v in box), thr)
            vol.mask.upload_view(padded[1:, 1:, 1:])
            vol.crop_mask(tuple(int(v) for v in box))
            assert np.array_equal(vol.download_mask(), host[1:, 1:, 1:]), box


def test_headless_crop(ivxlib, tmp_path, capsys):
    from conftest import synth_volume
    from invesalius3_amd import headless
    from invesalius3_amd import project as prj
    img = synth_volume((12, 20, 28), seed=31)
    p = prj.Project(name="Synth", spacing=(0.5, 0.5, 1.0), threshold_range=(int(img.min()), int(img.max())))
    p.matrix = img
    path, saved = tmp_path / "synth.inv3", tmp_path / "out.inv3"
    prj.save_inv3(path, p)
    lo, hi, box = max(int(np.median(img)) + 1000, 0), 3071, (4, 20, 2, 9, 3, 7)
    assert headless.main([str(a) for a in [path, "--threshold", lo, hi, "--crop", *box, "--save", saved]]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = np.ones(tuple(s + 1 for s in img.shape), np.uint8)
    want[1:, 1:, 1:] = np.where((img >= lo) & (img <= hi), 255, 0)
    R.crop_mask(want, img, box, (lo, hi))
    assert res["crop"] == {"limits": list(box)} and res["mask_voxels"] == int((want[1:, 1:, 1:] >= 127).sum()) > 0
    q = prj.open_inv3(saved)
    try:
        assert np.array_equal(q.masks[0].interior, want[1:, 1:, 1:])
    finally:
        q.close()
