"""GPU: the slice display -- slice_.get_slices, its five stage functions and DeviceVolume.show_slice against the
restatement of rules R1 - R7 (tests/_slice_display_ref.py) applied to the outputs of the existing get_image_slice /
get_mask_slice.  Every comparison is np.array_equal."""
import gc
import os

import numpy as np
import pytest

import _slice_display_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (33, 65, 67)
ORIENTATIONS = ("AXIAL", "CORONAL", "SAGITAL")
MASK_BYTES = np.array([0, 1, 2, 3, 127, 252, 253, 254, 255], np.uint8)
THR = (226, 3071)
# ww of 1, 255.5 and 65535 with wl at both ends of int16 (both clamps of R1 act), and two everyday windows
WINDOWS = [(1.0, -32768.0), (1.0, 32767.0), (255.5, -32768.0), (255.5, 32767.0), (65535.0, -32768.0), (65535.0, 32767.0),
           (255.5, 127.25), (2000.0, 300.0)]
EVERY_AUX = {k: ((k % 7) / 6, (k % 5) / 4, (k % 3) / 2, (k % 11) / 10) for k in range(256)}


def _specials():
    """the int16 ends and values on both sides of lo and hi of every window"""
    out = [-32768, -32767, 32766, 32767, 0, -1, 1]
    for ww, wl in WINDOWS:
        for edge in (wl - ww / 2, wl - ww / 2 + ww):
            e = int(min(max(edge, -32768.0), 32767.0))
            out += [e - 1, e, e + 1]
    return np.clip(np.array(out), -32768, 32767).astype(np.int16)


def _image(shape, seed=7):
    rng = np.random.default_rng(seed)
    img = rng.integers(-1200, 3300, shape).astype(np.int16)
    flat = img.reshape(-1)
    sp = _specials()
    at = np.arange(0, flat.size, 3)  # every third voxel is a special value, in turn
    flat[at] = np.resize(sp, at.size)
    return img


def _mask(shape, seed=8, flags=1):
    rng = np.random.default_rng(seed)
    m = np.zeros(tuple(s + 1 for s in shape), np.uint8)
    m[1:, 1:, 1:] = rng.choice(MASK_BYTES, size=shape)
    m[1:, 0, 0] = m[0, 1:, 0] = m[0, 0, 1:] = flags
    return m


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "ref_slicedisplay.npz"))


@pytest.fixture(scope="module")
def vol():
    """(image, padded mask with every flag 1, marker matrix) -- never written by a test (copies are)"""
    img, m = _image(SHAPE), _mask(SHAPE)
    markers = np.random.default_rng(9).integers(0, 3, SHAPE).astype(np.uint8)
    for a in (img, m, markers):
        a.setflags(write=False)
    return img, m, markers


@pytest.fixture(autouse=True)
def _registry_returns_to_what_it_was(ivxlib):
    from invesalius3_amd import resident
    before = resident.count()
    yield
    resident.set_check(False)
    gc.collect()
    assert resident.count() == before


def _plane(a, ori, n):
    return a[n] if ori == "AXIAL" else (a[:, n, :] if ori == "CORONAL" else a[:, :, n])


def _nodes(G, s):
    return [(float(v), tuple(int(c) for c in col)) for v, col in zip(G["nodes_%d_values" % s], G["nodes_%d_colours" % s])]


def _want(state, image2d, mask2d, aux2d, image_range, aux_colours=None):
    """the restatement on what get_image_slice / get_mask_slice returned"""
    nodes = None if state.nodes is None else [(n.value, n.colour) for n in state.nodes]
    return R.get_slices(image2d, mask2d, aux2d, mode=state.from_, ww=state.window_width, wl=state.window_level,
                        ranges=(state.saturation_range, state.hue_range, state.value_range), image_range=image_range,
                        values=state.values, nodes=nodes, mask_colour=state.mask_colour, opacity=state.opacity, aux_colours=aux_colours)


def _range(img):
    return img.min(), img.max()


# ---- widths, heights, windows: the vector path, its tail and unaligned rows ---------------------------------------------------------------
@pytest.mark.parametrize("h", [1, 2, 33])
def test_widths_heights_and_windows(ivxlib, h):
    from invesalius3_amd import slice_
    from invesalius3_amd import slice_display as D
    for w in (1, 3, 4, 5, 63, 64, 65, 257):
        img = _image((2, h, w), seed=w)
        m = _mask((2, h, w), seed=w + 1)
        for k, (ww, wl) in enumerate(WINDOWS if w in (5, 64, 257) else WINDOWS[k_for(w):k_for(w) + 2]):
            st = D.DisplayState(window_width=ww, window_level=wl, opacity=(0.0, 0.4, 1.0)[k % 3], mask_colour=D.MASK_COLOUR[k % 9])
            st.set_colour_table(list(D.SLICE_COLOR_TABLE)[k % 7])
            got = slice_.get_slices(img, m, "AXIAL", 1, 1, st)  # mask rows of pitch w + 1: aligned and unaligned rows
            assert got.shape == (h, w, 3) and got.dtype == np.uint8
            assert np.array_equal(got, _want(st, img[1], m[2, 1:, 1:], None, _range(img))), (h, w, ww, wl)
            # dense operands: every row of a width that is a multiple of 4 takes the dword loads and stores
            p, blob = D.build(st, D.IMG_I16, D.ST_ALL, image_range=_range(img), have_mask=True)
            dense = np.ascontiguousarray(m[2, 1:, 1:])
            assert np.array_equal(D.run(p, blob, img[1], dense, None, h, w), got)


def k_for(w):
    return {1: 0, 3: 2, 4: 4, 63: 6, 65: 1}[w]


# ---- the volume, all orientations, every colour mode ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ori,n", [("AXIAL", 16), ("CORONAL", 64), ("SAGITAL", 33), ("SAGITAL", 0)])
def test_colour_modes_on_the_volume(ivxlib, vol, G, ori, n):
    from invesalius3_amd import slice_
    from invesalius3_amd import slice_display as D
    img, m, _ = vol
    i2, m2 = _plane(img, ori, n), _plane(m[1:, 1:, 1:], ori, n)
    assert set(MASK_BYTES) <= set(np.unique(m2))
    states = []
    for k, name in enumerate(D.SLICE_COLOR_TABLE):  # all seven HSV tables
        st = D.DisplayState(window_width=WINDOWS[k][0], window_level=WINDOWS[k][1], opacity=(0.0, 0.4, 1.0)[k % 3])
        st.set_colour_table(name)
        states.append(st)
    for k in (0, 5):  # two plists
        for ww, wl in ((2000.0, 300.0), (1.0, 32767.0), (65535.0, -32768.0)):
            st = D.DisplayState(window_width=ww, window_level=wl)
            st.set_plist(G["plist_%d" % k])
            states.append(st)
    for s in range(3):  # 2, 3 and 16 nodes (two of them at one value)
        st = D.DisplayState(mask_colour=D.MASK_COLOUR[s + 1], opacity=1.0)
        st.set_widget_nodes(_nodes(G, s))
        states.append(st)
        moved = D.DisplayState()
        moved.set_widget_nodes(_nodes(G, s))
        D.update_wwwl_widget_nodes(moved.nodes, 900.5, 77.25)
        states.append(moved)
    assert len({len(_nodes(G, s)) for s in range(3)} & {2, 3, 16}) == 3
    for st in states:
        got = slice_.get_slices(img, m, ori, n, 1, st)
        assert np.array_equal(got, _want(st, i2, m2, None, _range(img))), (ori, st.from_, st.window_width, st.window_level)


def test_table_range_that_collapses(ivxlib, vol):
    from invesalius3_amd import slice_
    from invesalius3_amd import slice_display as D
    img, m, _ = vol
    for ww, wl, rng_ in ((1.0, -32768.0, None), (255.5, 127.25, (np.int16(5), np.int16(5))), (2.0, -32768.0, None)):
        rng_ = _range(img) if rng_ is None else rng_
        tmin, tmax = R.table_range(rng_[0], rng_[1], ww, wl)
        assert tmin == tmax
        for name in ("Rainbow", "Inverse Gray"):
            st = D.DisplayState(window_width=ww, window_level=wl)
            st.set_colour_table(name)
            got = slice_.get_slices(img, None, "CORONAL", 3, 1, st, image_range=rng_)
            assert np.array_equal(got, _want(st, img[:, 3, :], None, None, rng_))


# ---- the mask: shown, not shown, none; the lazy threshold ------------------------------------------------------------------------------------
def test_mask_states(ivxlib, vol):
    from invesalius3_amd import slice_
    from invesalius3_amd import slice_display as D
    img, m, _ = vol
    st = D.DisplayState(window_width=2000.0, window_level=300.0)
    bare = _want(st, img[:, :, 7], None, None, _range(img))
    assert np.array_equal(slice_.get_slices(img, None, "SAGITAL", 7, 1, st), bare)
    st.mask_shown = False
    assert np.array_equal(slice_.get_slices(img, m, "SAGITAL", 7, 1, st), bare)
    st.mask_shown = True
    for op in (0.0, 0.4, 1.0):
        st.opacity = op
        got = slice_.get_slices(img, m, "SAGITAL", 7, 1, st)
        assert np.array_equal(got, _want(st, img[:, :, 7], m[1:, 1:, 8], None, _range(img)))
        if op == 0.0:  # a transparent overlay still maps 255 to 254 (R7)
            assert np.array_equal(got, R.blend(bare, np.zeros(bare.shape[:2] + (4,), np.uint8))) and bare.max() == 255 and got.max() == 254


@pytest.mark.parametrize("ori,n", [("AXIAL", 5), ("CORONAL", 0), ("SAGITAL", 66)])
def test_lazy_threshold_of_a_stale_slice(ivxlib, vol, ori, n):
    from invesalius3_amd import slice_
    from invesalius3_amd import slice_display as D
    img, m, _ = vol
    stale = m.copy()
    stale[1:, 0, 0] = stale[0, 1:, 0] = stale[0, 0, 1:] = 0
    mine, theirs = stale.copy(), stale.copy()
    st = D.DisplayState(window_width=2000.0, window_level=300.0)
    got = slice_.get_slices(img, mine, ori, n, 1, st, threshold_range=THR)
    m2 = slice_.get_mask_slice(theirs, img, ori, n, THR)  # the existing path
    assert np.array_equal(mine, theirs) and not np.array_equal(mine, stale)  # mask bytes and flag
    assert np.array_equal(got, _want(st, _plane(img, ori, n), m2, None, _range(img)))
    with pytest.raises(ValueError):
        slice_.get_slices(img, stale.copy(), ori, n, 1, st)


# ---- the aux overlays -------------------------------------------------------------------------------------------------------------------------
def test_aux_overlays(ivxlib, vol):
    from invesalius3_amd import slice_
    from invesalius3_amd import slice_display as D
    img, m, markers = vol
    select = m[1:, 1:, 1:]  # "SELECT" is a strided view of the mask (styles.py:2803)
    for ori, n in (("AXIAL", 2), ("CORONAL", 31), ("SAGITAL", 65)):
        i2, m2 = _plane(img, ori, n), _plane(select, ori, n)
        st = D.DisplayState(window_width=400.0, window_level=40.0, to_show_aux="watershed")
        got = slice_.get_slices(img, m, ori, n, 1, st, aux_matrix=markers)
        assert np.array_equal(got, _want(st, i2, m2, _plane(markers, ori, n), _range(img), D.AUX_WATERSHED)), ori
        st.mask_shown = False  # the generic branch: the default dict, no mask overlay
        got = slice_.get_slices(img, m, ori, n, 1, st, aux_matrix=select)
        assert np.array_equal(got, _want(st, i2, None, m2, _range(img), D.AUX_DEFAULT)), ori
        st = D.DisplayState(window_width=400.0, window_level=40.0, to_show_aux="SELECT")
        got = slice_.get_slices(img, m, ori, n, 1, st, aux_matrix=select)
        assert np.array_equal(got, _want(st, i2, m2, m2, _range(img), D.AUX_DEFAULT)), ori
        st.aux_colours = {"SELECT": EVERY_AUX}  # a 256-entry dict
        got = slice_.get_slices(img, m, ori, n, 1, st, aux_matrix=select)
        assert np.array_equal(got, _want(st, i2, m2, m2, _range(img), EVERY_AUX)), ori
        # no current mask: no aux overlay either (slice_.py:800-816)
        assert np.array_equal(slice_.get_slices(img, None, ori, n, 1, st, aux_matrix=select), _want(st, i2, None, None, _range(img)))
    with pytest.raises(ValueError):
        st.aux_colours = {"SELECT": {1: (0, 0, 0, 0)}}
        slice_.get_slices(img, m, "AXIAL", 0, 1, st, aux_matrix=select)


# ---- projections --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("projection", ["MaxIP", "MinIP", "MeanIP", "MIDA", "CONTOUR_MIP"])
def test_projections(ivxlib, vol, projection):
    from invesalius3_amd import slice_
    from invesalius3_amd import slice_display as D
    img, m, _ = vol
    tp = getattr(slice_, "PROJECTION_" + projection)
    for ori, n in (("AXIAL", 3), ("CORONAL", 20), ("SAGITAL", 60)):
        for number, inverted in ((1, False), (5, False), (5, True)):
            st = D.DisplayState(window_width=700.5, window_level=250.0)
            st.set_colour_table("Ocean")
            i2 = slice_.get_image_slice(img, ori, n, number, inverted, 1.0, tp, st.window_level)
            assert i2.dtype == (np.float64 if projection == "MeanIP" else np.int16)
            got = slice_.get_slices(img, m, ori, n, number, st, inverted=inverted, type_projection=tp)
            assert np.array_equal(got, _want(st, i2, _plane(m[1:, 1:, 1:], ori, n), None, _range(img))), (ori, number, inverted)


def test_a_reoriented_view(ivxlib, vol):
    from invesalius3_amd import slice_
    from invesalius3_amd import slice_display as D
    img, m, _ = vol
    q, spacing = (0.9659258262890683, 0.0, 0.25881904510252074, 0.0), (0.5, 0.75, 2.0)
    center = [s * d / 2.0 for d, s in zip(SHAPE[::-1], spacing)]
    st = D.DisplayState(window_width=2000.0, window_level=300.0)
    for tp, number in ((slice_.PROJECTION_NORMAL, 1), (slice_.PROJECTION_MaxIP, 5)):
        i2 = slice_.get_image_slice(img, "AXIAL", 10, number, False, 1.0, tp, st.window_level, q, center, spacing)
        got = slice_.get_slices(img, m, "AXIAL", 10, number, st, type_projection=tp, q_orientation=q, center=center, spacing=spacing)
        assert np.array_equal(got, _want(st, i2, m[11, 1:, 1:], None, _range(img)))
        assert not np.array_equal(i2, img[10])


# ---- the five seams, one stage bit each ---------------------------------------------------------------------------------------------------------
def test_each_stage_alone(ivxlib, vol, G):
    from invesalius3_amd import slice_
    from invesalius3_amd import slice_display as D
    img, m, markers = vol
    i2, m2, a2 = img[:, :, 40], m[1:, 1:, 41], markers[:, :, 40]
    mean = i2.astype(np.float64) / 3.0 + 0.125
    for ww, wl in WINDOWS:
        st = D.DisplayState(window_width=ww, window_level=wl)
        st.set_colour_table("Rainbow")
        grey = slice_.do_ww_wl(i2, st)  # R1
        assert np.array_equal(grey, R.ww_wl(i2, R.OTHER, ww, wl))
        assert np.array_equal(slice_.do_ww_wl(mean, st), R.ww_wl(mean, R.OTHER, ww, wl))  # the float64 path
        tmin, tmax = R.table_range(*_range(img), ww, wl)
        col = slice_.do_colour_image(grey, st, _range(img))  # R2
        assert np.array_equal(col, R.colour_image(grey[..., 0], R.hsv_table(st.saturation_range, st.hue_range, st.value_range), tmin, tmax))
        st.set_plist(G["plist_3"])  # R3, and R2 the identity
        pl = slice_.do_ww_wl(i2, st)
        assert np.array_equal(pl, R.ww_wl(i2, R.PLIST, ww, wl, values=st.values)) and slice_.do_colour_image(pl, st, None) is pl
    st = D.DisplayState()
    st.set_widget_nodes(_nodes(G, 2))  # R4
    assert np.array_equal(slice_.do_ww_wl(i2, st), R.widget_colour(i2, _nodes(G, 2)))
    assert np.array_equal(slice_.do_ww_wl(mean, st), R.widget_colour(mean, _nodes(G, 2)))
    with pytest.raises(ValueError):
        slice_.do_ww_wl(i2, D.DisplayState(window_width=0.0))
    for op in (0.0, 0.4, 1.0):  # R5
        st = D.DisplayState(mask_colour=D.MASK_COLOUR[4], opacity=op)
        over = slice_.do_colour_mask(m2, st)
        assert over.shape == m2.shape + (4,) and np.array_equal(over, R.colour_mask(m2, st.mask_colour, op))
        assert np.array_equal(slice_.do_blend(col, over), R.blend(col, over))  # R7
    for colours, src in ((D.AUX_WATERSHED, a2), (D.AUX_DEFAULT, m2), (EVERY_AUX, m2), ({0: (1.0, 0.5, 0.25, 1.0)}, a2)):  # R6
        over = slice_.do_custom_colour(src, colours)
        assert np.array_equal(over, R.custom_colour(src, colours))
        assert np.array_equal(slice_.do_blend(col, over), R.blend(col, over))
    rng = np.random.default_rng(3)
    base, over = rng.integers(0, 256, (33, 65, 3)).astype(np.uint8), rng.integers(0, 256, (33, 65, 4)).astype(np.uint8)
    assert np.array_equal(slice_.do_blend(base, over), R.blend(base, over))


# ---- bound and unbound, and what crosses the link --------------------------------------------------------------------------------------------------
def _xfer():
    from invesalius3_amd import resident
    s = resident.transfer_stats()
    return s["h2d_bytes"], s["d2h_bytes"]


def test_bound_equals_unbound_and_the_picture_crosses_once(ivxlib, vol):
    from invesalius3_amd import mask as mk
    from invesalius3_amd import resident, slice_
    from invesalius3_amd import slice_display as D
    img, m, markers = vol
    img, m, markers = img.copy(), m.copy(), markers.copy()
    m[6, 0, 0] = m[0, 7, 0] = m[0, 0, 8] = 0  # one stale slice per orientation
    st = D.DisplayState(window_width=2000.0, window_level=300.0, to_show_aux="watershed")
    st.set_colour_table("Hue")
    cases = [("AXIAL", 5), ("CORONAL", 6), ("SAGITAL", 7), ("AXIAL", 20), ("CORONAL", 21), ("SAGITAL", 22)]
    unbound_m = m.copy()
    unbound = [slice_.get_slices(img, unbound_m, o, n, 1, st, threshold_range=THR, aux_matrix=markers) for o, n in cases]
    rng_ = _range(img)
    with slice_.bind_image(img), mk.bind_matrix(m), resident.bind(markers):
        resident.set_check(True)  # every use compares host and mirror first
        bound = [slice_.get_slices(img, m, o, n, 1, st, threshold_range=THR, aux_matrix=markers, image_range=rng_) for o, n in cases]
        resident.set_check(False)
        assert np.array_equal(m, unbound_m)
        for a, b, c in zip(bound, unbound, cases):
            assert np.array_equal(a, b), c
        # the counters: nothing of image, mask or aux goes host -> device -- the tables block is all -- and exactly the picture
        # comes back
        for o, n in cases:
            h, w = _plane(img, o, n).shape
            up0, down0 = _xfer()
            slice_.get_slices(img, m, o, n, 1, st, aux_matrix=markers, image_range=rng_)
            up1, down1 = _xfer()
            assert up1 - up0 == 3072, (o, up1 - up0)
            assert down1 - down0 == h * w * 3, (o, down1 - down0)
    # unbound: the three slices, never the volume
    h, w = _plane(img, "SAGITAL", 22).shape
    up0, _ = _xfer()
    slice_.get_slices(img, m, "SAGITAL", 22, 1, st, aux_matrix=markers, image_range=rng_)
    assert _xfer()[0] - up0 == 3072 + h * w * 4


# ---- the device-resident form --------------------------------------------------------------------------------------------------------------------------
def test_device_volume_show_slice_equals_the_host_form(ivxlib, vol, G):
    from invesalius3_amd import _lib as L
    from invesalius3_amd import slice_
    from invesalius3_amd import slice_display as D
    from invesalius3_amd.device import DeviceBuffer, DeviceVolume
    img, m, markers = vol
    states = []
    st = D.DisplayState(window_width=2000.0, window_level=300.0, to_show_aux="watershed")
    st.set_colour_table("Desert")
    states.append(st)
    st = D.DisplayState(window_width=80.0, window_level=32767.0, to_show_aux="SELECT", opacity=1.0)
    st.set_plist(G["plist_7"])
    states.append(st)
    st = D.DisplayState(mask_shown=False)
    st.set_widget_nodes(_nodes(G, 2))
    states.append(st)
    with DeviceVolume(img) as dv:
        dv.mask.upload_view(m[1:, 1:, 1:])
        d_markers = DeviceBuffer(markers.size)
        d_markers.upload(markers)
        for st in states:
            for ori, n in (("AXIAL", 0), ("AXIAL", 32), ("CORONAL", 33), ("SAGITAL", 66), ("SAGITAL", 1)):
                aux_host, aux_dev = (markers, d_markers) if st.to_show_aux == "watershed" else (m[1:, 1:, 1:], dv.mask)
                want = slice_.get_slices(img, m, ori, n, 1, st, aux_matrix=aux_host if st.to_show_aux else None)
                got = dv.show_slice(ori, n, st, aux=aux_dev if st.to_show_aux else None)
                assert np.array_equal(got, want), (ori, n, st.from_)
                held = dv.show_slice(ori, n, st, aux=aux_dev if st.to_show_aux else None, download=False)
                dv.sync()
                assert np.array_equal(held.download(want.shape, np.uint8), want)
        # the dense device output of the projection kernels goes in as it is: MaxIP (int16) and MeanIP (float64) of the volume
        st = states[0]
        for op, tp, dt in ((L.MIP_MAX, slice_.PROJECTION_MaxIP, np.int16), (L.MIP_MEAN, slice_.PROJECTION_MeanIP, np.float64)):
            for ax, ori in enumerate(ORIENTATIONS):
                h, w = (s for k, s in enumerate(SHAPE) if k != ax)
                proj = DeviceBuffer(h * w * np.dtype(dt).itemsize)
                dv.project(ax, op, proj)
                got = dv.show_slice(ori, 0, st, image=proj, image_dtype=dt, aux=d_markers)
                want = slice_.get_slices(img, m, ori, 0, SHAPE[ax], st, type_projection=tp, aux_matrix=markers)
                assert np.array_equal(got, want), (ori, tp)
                proj.close()
        d_markers.close()
