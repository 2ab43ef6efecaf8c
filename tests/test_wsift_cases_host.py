"""The case table of _wsift_cases.py, checked without a GPU: every row's flood, by the serial reference and the plain census of
its cost map, reaches the branch of the IFT watershed's level chain (csrc/k_wsift.hip) that the row is named for, and the
census itself counts three hand-countable volumes right.  The GPU half is test_gpu_wsift_chain.py."""
import numpy as np
import pytest
from scipy.ndimage import generate_binary_structure

import _wsift_cases as W


def _census(oracle, img, mk, s):
    lab, cost = oracle.watershed_ift_clean(img, mk, s, want_cost=True)
    assert cost.max() < 0xFFFF  # every voxel is reached
    return W.census(img, mk, s, cost)


@pytest.mark.parametrize("case", W.WSIFT_CHAIN_CASES, ids=W.CASE_IDS)
def test_case_reaches_its_branch(oracle, case):
    img, mk, s = W.build_case(case)
    assert img.dtype == np.uint16 and mk.dtype == np.int16 and img.ndim == case["ndim"] and img.size <= 282240
    cen = _census(oracle, img, mk, s)
    print(case["id"], {k: v for k, v in cen.items() if k != "level_counts"})
    W.check_need(case, cen, img.shape)
    for k, v in case["seen"].items():  # the counts recorded in the table are the ones this construction gives
        assert cen[k] == v, (case["id"], k, cen[k], v)


def test_the_switches_the_table_names():
    """the arithmetic behind the ids, from the constants restated in _wsift_cases.py"""
    by = {c["id"]: c for c in W.WSIFT_CHAIN_CASES}
    # k_ws_rank: 1024 lanes, chunk = ceil(words / 1024): 1024 words -> one word a lane, 1025 -> two, the 513th lane partly filled
    assert [-(-by[i]["need"]["rank_words0"] // W.RANK_LANES) for i in ("rank-1024w", "rank-1025w", "used-8192w", "used-8193w")] == [1, 2, 8, 9]
    # the used-key bitmap of the first level above 0: LDS up to 8192 words
    words = {i: W.bitmap_words(by[i]["need"]["stamps1"]) for i in ("stamps-cross", "stamps-8192w", "stamps-8193w")}
    assert words == {"stamps-cross": 8192, "stamps-8192w": 8192, "stamps-8193w": 8193}
    assert by["stamps-8192w"]["need"]["stamps1"] - 1 == 8191 * 32 + 31 and by["stamps-8193w"]["need"]["stamps1"] - 1 == 8192 * 32
    # stamps-cross: 2^18 - 4 stamps before the first level, at least one more per level, at least 6 levels: the last ones see
    # more than 2^18 stamps, whatever the code under test reports
    assert by["stamps-cross"]["need"]["stamps1"] + by["stamps-cross"]["need"]["levels"] - 1 > W.USED_LDS_STAMPS
    # the issue's dense rows: already level 0 alone (one stamp per run of labels, at least one) puts every later level of
    # used-8192w / used-8193w past the switch; used-cross needs its levels for that
    assert by["used-8192w"]["args"][1] + 1 > W.USED_LDS_STAMPS and by["used-cross"]["args"][1] + 1 + 6 - 1 > W.USED_LDS_STAMPS
    # three bucket workgroups, the last one partial
    assert 2 * W.BUCKET_VOXELS < 12 * 40 * 70 < 3 * W.BUCKET_VOXELS


def test_dense_stamps_builds_what_it_says():
    img, mk = W.dense_stamps((3, 5, 7), 40, seed=5)
    lab = mk.ravel()[mk.ravel() != 0]
    assert lab.size == 24 and 1 + int((lab[1:] != lab[:-1]).sum()) == 16 and set(lab.tolist()) <= {1, 2, 3}
    assert mk.ravel()[[0, 2, 8, 36, 104]].all() and mk.ravel()[1] == 0
    img2, mk2 = W.dense_markers((3, 5, 7), 11, seed=5)
    assert int((mk2 != 0).sum()) == 11 and mk2[-1, -1, -1] != 0 and img2.max() < 40


# ---- the census on volumes one can count by hand -------------------------------------------------------------------------
def test_census_of_a_line(oracle):
    """I = 0 5 5 7 2 0, markers at both ends.  Costs 0 5 5 5 2 0.  Voxel 1 is an entry (parent 0, arc 5), voxel 2 is not (its
    neighbours cost 5 like itself): the one zone, touched by the entries 1 and 3; voxel 3 enters from 4 (arc 5), voxel 4 from
    the marker 5 (arc 2) and touches no zone."""
    img = np.array([[[0, 5, 5, 7, 2, 0]]], np.uint16)
    mk = np.array([[[1, 0, 0, 0, 0, 2]]], np.int16)
    s = generate_binary_structure(3, 1)
    lab, cost = oracle.watershed_ift_clean(img, mk, s, want_cost=True)
    assert cost.ravel().tolist() == [0, 5, 5, 5, 2, 0]
    assert W.census(img, mk, s, cost) == dict(markers=2, entries=3, levels=2, max_level=5, level_counts={2: 1, 5: 2},
                                              parents_hist=[3, 0, 0], zones_hist=[1, 2, 0, 0, 0], marker_classes=2,
                                              top_stamp_is_key=False)  # (the lowest level's entry hangs on the LAST marker)


def test_census_of_the_reference_fixture(oracle):
    """the 5x5x5 fixture of test_reference_fixture: a cube of 100 in a shell of 0, one marker in each -- both parts are flat,
    every cost is 0, nothing but the markers is an entry"""
    image = np.zeros((5, 5, 5), np.uint16)
    image[1:4, 1:4, 1:4] = 100
    mk = np.zeros((5, 5, 5), np.int16)
    mk[2, 2, 2], mk[0, 0, 0] = 1, 2
    s = generate_binary_structure(3, 1)
    lab, cost = oracle.watershed_ift_clean(image, mk, s, want_cost=True)
    assert not cost.any() and (lab == 1).sum() == 27 and (lab == 2).sum() == 98
    assert W.census(image, mk, s, cost) == dict(markers=2, entries=0, levels=0, max_level=0, level_counts={}, parents_hist=[0, 0, 0],
                                                zones_hist=[0, 0, 0, 0, 0], marker_classes=2, top_stamp_is_key=False)


def test_census_of_a_single_star(oracle):
    """3x3x5 of wall (1000) around one star: centre 22 = (1,1,2) and its arms 23, 7, 37, 17, 27 at 10, the marker 21 = (1,1,1)
    at 0.  The centre enters at cost 10 from the marker and touches five one-voxel zones (the arms).  The walls cost 990; the
    13 of them next to an arm BY LINEAR INDEX (2 6 8 12 16 18 24 26 28 32 36 38 42) are entries, with 1 / 2 / 3 arms for
    parents (6 16 24 26 36 / 2 8 18 28 38 42 / 12 32), and the other 25 walls are one zone that each of the 13 touches."""
    img = np.full((3, 3, 5), 1000, np.uint16)
    for z, y, x in ((1, 1, 2), (1, 1, 3), (0, 1, 2), (2, 1, 2), (1, 0, 2), (1, 2, 2)):
        img[z, y, x] = 10
    img[1, 1, 1] = 0
    mk = np.zeros(img.shape, np.int16)
    mk[1, 1, 1] = 3
    s = generate_binary_structure(3, 1)
    lab, cost = oracle.watershed_ift_clean(img, mk, s, want_cost=True)
    assert sorted(set(cost.ravel().tolist())) == [0, 10, 990] and (cost == 10).sum() == 6
    assert W.census(img, mk, s, cost) == dict(markers=1, entries=14, levels=2, max_level=990, level_counts={10: 1, 990: 13},
                                              parents_hist=[6, 6, 2], zones_hist=[0, 13, 0, 0, 1], marker_classes=1,
                                              top_stamp_is_key=True)
