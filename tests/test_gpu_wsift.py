"""The IFT watershed flood on the GPU (csrc/k_wsift.hip) against (i) the defect-free C statement of scipy's algorithm
(oracle/ivx_oracle_wsz.c) -- bit for bit, labels AND minimax cost map -- and (ii) live scipy.ndimage.watershed_ift, the
function the reference calls (invesalius/data/watershed_process.py:44-46,54-57): equal wherever scipy's linked-list
defect did not fire (oracle.watershed_ift_events reports no late / lost pops), mismatching voxels counted otherwise."""
import numpy as np
import pytest
from scipy import ndimage
from scipy.ndimage import generate_binary_structure

from conftest import synth_volume

pytestmark = pytest.mark.gpu


def _lut(x, W, L):
    return np.piecewise(x, [x <= (L - 0.5 - (W - 1) / 2.0), x > (L - 0.5 + (W - 1) / 2.0)],
                        [0, W, lambda v: ((v - (L - 0.5)) / (W - 1) + 0.5) * W]).astype(np.uint16)


def _markers(img):
    mk = np.zeros(img.shape, np.int16)
    d, h, w = img.shape
    z, y, x = np.unravel_index(int(np.argmax(img)), img.shape)
    z, y, x = min(max(z, 2), d - 3), min(max(y, 2), h - 3), min(max(x, 2), w - 3)
    for cz in (0, max(d - 5, 0)):
        for cy in (0, h - 5):
            for cx in (0, w - 5):
                mk[cz:cz + 5, cy:cy + 5, cx:cx + 5] = 2
    mk[max(z - 2, 0):z + 3, y - 2:y + 3, x - 2:x + 3] = 1
    return mk


def test_reference_fixture(ivxlib):
    """tests/test_segmentation_tools.py:170-213 through the IFT branch: 27 voxels label 1, 98 label 2 (== scipy)."""
    from invesalius3_amd import watershed_process as wp
    image = np.zeros((5, 5, 5), dtype=np.int16)
    image[1:4, 1:4, 1:4] = 100
    markers = np.zeros((5, 5, 5), dtype=np.int16)
    markers[2, 2, 2] = 1
    markers[0, 0, 0] = 2
    cost = (image - image.min()).astype("uint16")
    s = generate_binary_structure(3, 1)
    got = wp.watershed_ift(cost, markers, s)
    assert np.array_equal(got, ndimage.watershed_ift(cost, markers, s))
    assert (got == 1).sum() == 27 and (got == 2).sum() == 98


def test_black_box_facts(ivxlib):
    from invesalius3_amd import watershed_process as wp
    line = np.array([[0, 0, 0], [1, 1, 1], [0, 0, 0]], np.uint8)
    for img, mk in (([0, 6, 5, 8], [1, 0, 0, 2]), ([0, 0, 0, 0, 0], [1, 0, 0, 0, 2]), ([0, 0, 0, 0, 0], [2, 0, 0, 0, 1])):
        a = np.array(img, np.uint16).reshape(1, -1)
        m = np.array(mk, np.int16).reshape(1, -1)
        assert np.array_equal(wp.watershed_ift(a, m, line), ndimage.watershed_ift(a, m, line))


def _cases(seed, n):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        nd = int(rng.choice([2, 3]))
        shape = tuple(int(v) for v in (rng.integers(1, 12, 3) if nd == 3 else rng.integers(1, 40, 2)))
        conn = int(rng.integers(1, nd + 1))
        hi = int(rng.choice([2, 4, 10, 60, 3000, 65535]))
        img = rng.integers(0, hi + 1, shape).astype(np.uint16)
        if rng.random() < 0.5:
            img[rng.random(shape) < 0.4] = 0
        if rng.random() < 0.3:
            img = ndimage.uniform_filter(img.astype(float), 3).astype(np.uint16)
        mk = np.zeros(shape, np.int16)
        nm = int(rng.integers(1, 8))
        mk.ravel()[rng.integers(0, img.size, nm)] = rng.choice(np.array([1, 2, 3], np.int16), nm)
        if rng.random() < 0.3 and img.size > 8:
            mk[tuple(slice(0, max(1, s // 2)) for s in shape)] = 2
        yield img, mk, generate_binary_structure(nd, conn)


def test_random_small_volumes(ivxlib, oracle):
    """labels and cost map == the defect-free oracle on every case; == live scipy on every case where scipy's
    unlink defect stayed harmless (no late pop, no lost element)."""
    from invesalius3_amd import watershed_process as wp
    n_scipy_equal = n_defect = 0
    for img, mk, s in _cases(11, 250):
        got, cost = wp.watershed_ift(img, mk, s, want_cost=True)
        exp, ecost = oracle.watershed_ift_clean(img, mk, s, want_cost=True)
        assert np.array_equal(cost.astype(np.uint32) | np.where(ecost == 0xFFFFFFFF, 0, 0).astype(np.uint32),
                              np.where(ecost == 0xFFFFFFFF, 0xFFFF, ecost)), "cost map"
        assert np.array_equal(got, exp), "labels vs defect-free oracle %s" % (img.shape,)
        sci = ndimage.watershed_ift(img, mk, s)
        f, ev = oracle.watershed_ift_events(img, mk, s)
        assert np.array_equal(f, sci)
        if ev[1] == 0 and ev[3] == 0:
            assert np.array_equal(got, sci), "scipy without defect events"
            n_scipy_equal += 1
        else:
            n_defect += 1
    assert n_scipy_equal > 150
    print("ift small: %d cases == scipy, %d cases with scipy defect events" % (n_scipy_equal, n_defect))


def test_uint8_int8_and_2d(ivxlib, oracle):
    from invesalius3_amd import watershed_process as wp
    rng = np.random.default_rng(3)
    img = rng.integers(0, 40, (20, 30)).astype(np.uint8)
    mk = np.zeros((20, 30), np.int8)
    mk[3, 4] = 1
    mk[15, 22] = 2
    for conn in (1, 2):
        s = generate_binary_structure(2, conn)
        got = wp.watershed_ift(img, mk, s)
        assert got.dtype == np.int8 and np.array_equal(got, oracle.watershed_ift_clean(img, mk, s))
    with pytest.raises(TypeError):
        wp.watershed_ift(img.astype(np.int16), mk, generate_binary_structure(2, 1))
    mk[0, 0] = -1
    with pytest.raises(TypeError):
        wp.watershed_ift(img, mk, generate_binary_structure(2, 1))


@pytest.mark.parametrize("n,mode,conn", [(48, "minshift", 1), (64, "minshift", 3), (64, "lut", 1), (96, "lut", 3),
                                         (96, "minshift", 2), (128, "lut", 3)])
def test_phantom_volumes(ivxlib, oracle, n, mode, conn):
    """noise + blobs phantom (conftest.synth_volume), both cost images of watershed_process.py, SURVEY 8(d) markers"""
    from conftest import synth_volume
    from invesalius3_amd import watershed_process as wp
    img = synth_volume((n, n, n), seed=5)
    mk = _markers(img)
    cost = (img - img.min()).astype(np.uint16) if mode == "minshift" else _lut(img, 400, 300)
    mk = mk.astype(np.int8) if mode == "minshift" else mk
    s = generate_binary_structure(3, conn)
    got, gcost, st = wp.watershed_ift(cost, mk, s, want_cost=True, want_stats=True)
    exp, ecost = oracle.watershed_ift_clean(cost, mk, s, want_cost=True)
    assert np.array_equal(gcost, ecost.astype(np.uint16)), "cost map"
    assert np.array_equal(got, exp), "labels vs defect-free oracle: %d voxels differ" % int((got != exp).sum())
    sci = ndimage.watershed_ift(cost, mk, s)
    f, ev = oracle.watershed_ift_events(cost, mk, s)
    assert np.array_equal(f, sci)
    mism = int((got != sci).sum())
    print("ift %d^3 %s conn %d: %s | vs live scipy: %d of %d voxels differ; scipy defect events (requeue, late, twice, lost) = %s"
          % (n, mode, conn, st, mism, got.size, ev))
    if ev[1] == 0 and ev[3] == 0:
        assert mism == 0
    assert mism <= got.size // 500  # the defect touches a handful of voxels, never the segmentation


def test_degenerate_inputs(ivxlib, oracle):
    """no voxels, one voxel, no markers, only markers, a 1-D line, maximal labels"""
    from invesalius3_amd import watershed_process as wp
    s = generate_binary_structure(3, 1)
    z = wp.watershed_ift(np.zeros((0, 4, 4), np.uint16), np.zeros((0, 4, 4), np.int16), s)
    assert z.shape == (0, 4, 4)
    one = wp.watershed_ift(np.array([[[7]]], np.uint16), np.array([[[3]]], np.int16), s)
    assert one.tolist() == [[[3]]]
    img = np.random.default_rng(0).integers(0, 50, (6, 7, 9)).astype(np.uint16)
    assert not wp.watershed_ift(img, np.zeros(img.shape, np.int16), s).any()          # nothing to flood from
    full = np.random.default_rng(1).integers(1, 5, img.shape).astype(np.int16)
    assert np.array_equal(wp.watershed_ift(img, full, s), full)                       # every voxel is its own marker
    line = np.array([[[0, 9, 3, 3, 8, 1, 1, 2]]], np.uint16)
    mk = np.zeros(line.shape, np.int16)
    mk[0, 0, 0], mk[0, 0, -1] = 32767, 1
    got = wp.watershed_ift(line, mk, s)
    assert np.array_equal(got, oracle.watershed_ift_clean(line, mk, s)) and np.array_equal(got, ndimage.watershed_ift(line, mk, s))
    assert got.max() == 32767


def test_millions_of_marker_voxels(ivxlib, oracle):
    """a brush-painted volume: more marker voxels than the default time-stamp table holds (the tables are re-sized and the
    flood starts over)"""
    from conftest import synth_volume
    from invesalius3_amd import watershed_process as wp
    img = synth_volume((176, 176, 176), seed=12)
    cost = (img - img.min()).astype(np.uint16)
    mk = np.zeros(img.shape, np.int8)
    mk[:, :120, :] = 1      # 3.7 M voxels of label 1 ...
    mk[:, 150:, :] = 2      # ... and 0.8 M of label 2: 4.5 M markers > 2^22
    s = generate_binary_structure(3, 1)
    got, st = wp.watershed_ift(cost, mk, s, want_stats=True)
    assert st["markers"] == int((mk != 0).sum()) > (1 << 22)
    assert np.array_equal(got, oracle.watershed_ift_clean(cost, mk, s))


@pytest.mark.parametrize("shape", [(20, 16, 64), (33, 32, 128), (17, 48, 192), (40, 64, 64), (3, 16, 128)])
@pytest.mark.parametrize("frac", ["0.9", "1.0", "0.3"])
def test_cost_levels_on_bit_planes_equal_the_serial_flood(ivxlib, oracle, monkeypatch, shape, frac):
    """The cost map's level floods (ivx_dev_ws_cost_levels, csrc/k_costlevels.hip: arc planes + scipy's linear-index
    neighbourhood on a flat bit array) followed by the relaxation of what is left: labels AND costs equal the serial,
    defect-free flood on volumes whose borders matter (one word / one tile wide, odd slice counts), whatever share of the
    voxels the levels take."""
    from invesalius3_amd import watershed_process as wp
    monkeypatch.setenv("IVX_WS_LEVELS_MIN", "0")
    monkeypatch.setenv("IVX_WS_LEVELS_FRAC", frac)
    rng = np.random.default_rng(hash(shape) & 0xffff)
    s6 = generate_binary_structure(3, 1)
    for trial in range(3):
        if trial == 0:
            img = rng.integers(0, 40, shape).astype(np.uint16)               # dense noise: the bulk connects at one level
        elif trial == 1:
            img = (synth_volume(shape, seed=trial + shape[0]) + 1024).astype(np.uint16)
        else:
            img = (rng.integers(0, 6, shape) * 50).astype(np.uint16)          # plateaus and cliffs
        mk = np.zeros(shape, np.int16)
        for lab in (1, 2, 3):
            for _ in range(3):
                z, y, x = (int(rng.integers(0, s)) for s in shape)
                mk[z, y, x] = lab
        mk[0, 0, 0], mk[-1, -1, -1] = 1, 2                                     # the corners the wrap-around arcs start from
        got, cost, st = wp.watershed_ift(img, mk, s6, want_cost=True, want_stats=True)
        want, wcost = oracle.watershed_ift_clean(img, mk, s6, want_cost=True)
        assert st["cost_levels"] > 0, st
        assert np.array_equal(cost.astype(np.uint32), wcost), (shape, frac, trial, int((cost != wcost).sum()))
        assert np.array_equal(got, want), (shape, frac, trial)
    monkeypatch.setenv("IVX_WS_LEVELS", "0")                                   # the relaxation alone: same answer
    got0 = wp.watershed_ift(img, mk, s6)
    assert np.array_equal(got0, want)
