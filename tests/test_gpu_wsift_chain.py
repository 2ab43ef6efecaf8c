"""The level chain of the IFT watershed (csrc/k_wsift.hip stages 3 to 5: entries by level, keys -> rank -> claim per level,
labels) on the cases of _wsift_cases.py, each built for one switch of the chain (test_wsift_cases_host.py proves on the CPU
that it gets there): link records with more than two parent words / more than three zones, the unlinked kernels that take over
when the records cannot be allocated, the used-key bitmap in LDS / per wave at 8192 | 8193 words, k_ws_rank at 1024 | 1025
words, bucket workgroups with levels on both sides of their LDS counters.  Labels and cost map against the defect-free serial
flood, bit for bit, and the flood's own statistics against the plain census of the reference's cost map."""
import itertools

import numpy as np
import pytest

import _wsift_cases as W
from test_gpu_wsift import _cases

pytestmark = pytest.mark.gpu

LINKS = [None, "0"]  # IVX_WS_LINKS unset: link records; "0": k_ws_keys / k_ws_claim / k_ws_bucket<..., true>
LINK_IDS = ["links", "nolinks"]
_BY_ID = {c["id"]: c for c in W.WSIFT_CHAIN_CASES}
_REF, _GOT = {}, {}


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def _ref(oracle, cid):
    """(image, markers, structure, reference labels, reference cost, census), computed once per case"""
    if cid not in _REF:
        img, mk, s = W.build_case(_BY_ID[cid])
        lab, cost = oracle.watershed_ift_clean(img, mk, s, want_cost=True)
        _REF[cid] = _frozen(img, mk, s, lab, cost) + (W.census(img, mk, s, cost),)
    return _REF[cid]


def _set_links(monkeypatch, links):
    monkeypatch.setenv("IVX_WS_LEVELS", "0")  # the cost map from the relaxation, with and without links
    if links is None:
        monkeypatch.delenv("IVX_WS_LINKS", raising=False)
    else:
        monkeypatch.setenv("IVX_WS_LINKS", links)


def _flood(oracle, monkeypatch, cid, links):
    """(labels, cost, stats) of the GPU flood, run once per (case, links)"""
    if (cid, links) not in _GOT:
        from invesalius3_amd import watershed_process as wp
        img, mk, s = _ref(oracle, cid)[:3]
        _set_links(monkeypatch, links)
        _GOT[cid, links] = wp.watershed_ift(img, mk, s, want_cost=True, want_stats=True)
    return _GOT[cid, links]


@pytest.mark.parametrize("links", LINKS, ids=LINK_IDS)
@pytest.mark.parametrize("cid", W.CASE_IDS)
def test_chain_case_equals_the_serial_flood(ivxlib, oracle, monkeypatch, cid, links):
    img, mk, s, exp, ecost, cen = _ref(oracle, cid)
    got, cost, st = _flood(oracle, monkeypatch, cid, links)
    print(cid, links, {k: st[k] for k in ("markers", "entries", "levels", "time_stamps")},
          {k: v for k, v in cen.items() if k != "level_counts"})
    assert got.dtype == mk.dtype and cost.dtype == np.uint16
    assert np.array_equal(cost.astype(np.uint32), ecost), "cost map: %d voxels differ" % int((cost != ecost).sum())
    assert np.array_equal(got, exp), "labels: %d voxels differ" % int((got != exp).sum())
    assert st["markers"] == cen["markers"]
    assert st["entries"] == cen["markers"] + cen["entries"]
    assert st["levels"] == cen["levels"] + 1
    assert st["time_stamps"] >= st["markers"] + cen["levels"]
    # level 0 issues one stamp per run of equal labels among the markers in raster order, every later level at least one and
    # at most one per entry
    first = cen["markers"] + cen["marker_classes"]
    assert first + cen["levels"] <= st["time_stamps"] <= first + cen["entries"]
    # which side of the used-key bitmap's switch, from the reference alone
    if cid in ("used-cross", "used-8192w"):
        assert cen["markers"] <= 2 ** 18
    if cid == "used-8193w":
        assert cen["markers"] > 2 ** 18
    if cid in ("stamps-cross", "stamps-8192w"):
        assert W.bitmap_words(first) == W.USED_LDS_WORDS
    if cid == "stamps-8193w":
        assert W.bitmap_words(first) == W.USED_LDS_WORDS + 1
    if cid in ("used-cross", "stamps-cross"):
        assert st["time_stamps"] > 2 ** 18


@pytest.mark.parametrize("cid", W.CASE_IDS)
def test_linked_and_unlinked_chain_agree(ivxlib, oracle, monkeypatch, cid):
    a, acost, ast = _flood(oracle, monkeypatch, cid, None)
    b, bcost, bst = _flood(oracle, monkeypatch, cid, "0")
    assert np.array_equal(a, b) and np.array_equal(acost, bcost)
    for k in ("time_stamps", "entries", "levels", "markers"):
        assert ast[k] == bst[k], (k, ast[k], bst[k])


@pytest.mark.parametrize("links", LINKS, ids=LINK_IDS)
def test_int8_markers_on_uint8_intensities(ivxlib, oracle, monkeypatch, links):
    from invesalius3_amd import watershed_process as wp
    img, mk, s, exp, ecost, _ = _ref(oracle, "checker")
    _set_links(monkeypatch, links)
    got, cost = wp.watershed_ift(img.astype(np.uint8), mk.astype(np.int8), s, want_cost=True)
    assert got.dtype == np.int8 and np.array_equal(got, exp.astype(np.int8)) and np.array_equal(cost.astype(np.uint32), ecost)
    assert np.array_equal(exp, oracle.watershed_ift_clean(img.astype(np.uint8), mk.astype(np.int8), s))


@pytest.mark.parametrize("links", LINKS, ids=LINK_IDS)
@pytest.mark.parametrize("dtype,hi", [(np.int8, 127), (np.int16, 32767)], ids=["int8-127", "int16-32767"])
def test_extreme_labels_survive_the_label_table(ivxlib, oracle, monkeypatch, dtype, hi, links):
    """the label table is int32 inside; the cast back must hold the largest label of the markers' type"""
    from invesalius3_amd import watershed_process as wp
    img, mk, s = _ref(oracle, "star-tiles")[:3]
    mk = np.where(mk == 0, 0, np.where(mk == 1, 1, hi)).astype(dtype)
    exp, ecost = oracle.watershed_ift_clean(img, mk, s, want_cost=True)
    _set_links(monkeypatch, links)
    got, cost = wp.watershed_ift(img, mk, s, want_cost=True)
    assert got.dtype == dtype and int(got.max()) == hi and int(got.min()) == 1
    assert np.array_equal(got, exp) and np.array_equal(cost.astype(np.uint32), ecost)


def test_random_small_volumes_without_links(ivxlib, oracle, monkeypatch):
    """the first 60 volumes of test_gpu_wsift.test_random_small_volumes through the unlinked kernels"""
    from invesalius3_amd import watershed_process as wp
    monkeypatch.setenv("IVX_WS_LINKS", "0")
    n = 0
    for img, mk, s in itertools.islice(_cases(11, 60), 60):
        got, cost = wp.watershed_ift(img, mk, s, want_cost=True)
        exp, ecost = oracle.watershed_ift_clean(img, mk, s, want_cost=True)
        assert np.array_equal(cost.astype(np.uint32), np.where(ecost == 0xFFFFFFFF, 0xFFFF, ecost)), ("cost map", n, img.shape)
        assert np.array_equal(got, exp), ("labels", n, img.shape)
        n += 1
    assert n == 60


def test_do_watershed_in_one_call_without_links(ivxlib, oracle, monkeypatch, tmp_path):
    """do_watershed's IFT branch on the min-shifted image (int8 markers, the uint8 output of k_ws_labels) through the unlinked
    kernels == its stages == the serial flood"""
    import warnings

    from invesalius3_amd import watershed_process as wp
    img, mk, s, exp = _ref(oracle, "star-3blocks")[:4]
    image = img.astype(np.int16)
    assert image.min() == 0  # the min-shift leaves the case as the census saw it
    _set_links(monkeypatch, "0")
    tfile = str(tmp_path / "ws.dat")
    np.memmap(tfile, shape=image.shape, dtype="uint8", mode="w+").flush()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", wp.IftDeviationWarning)
        wp.do_watershed(image, mk, tfile, image.shape, s, "Watershed IFT", (3, 3, 3), False, 300, 400, None)
    got = np.array(np.memmap(tfile, shape=image.shape, dtype="uint8", mode="r"))
    cost = wp.cost_image(image, False, 300, 400, 0)
    assert np.array_equal(cost, img)
    want = wp.watershed_ift(cost, mk.astype(np.int8), s)
    assert np.array_equal(got, want.astype(np.uint8))
    assert np.array_equal(got, exp.astype(np.uint8)) and set(np.unique(got).tolist()) == {1, 2, 3}
