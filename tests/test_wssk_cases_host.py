"""The case table of _wssk_cases.py, checked without a GPU: the plain reference equals the serial flood on every case, the census
puts every case on the path of the GUI-default watershed's level chain (csrc/k_wssk.hip) that it is named for, the constants
and conditions restated there are the ones the .hip file defines, and the census counts three hand-countable volumes right.  The
GPU half is test_gpu_wssk_chain.py."""
import os
import re

import numpy as np
import pytest
from scipy.ndimage import generate_binary_structure

import _wssk_cases as W

HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "invesalius3_amd", "csrc")


@pytest.mark.parametrize("case", W.CASES, ids=W.CASE_IDS)
def test_case_reaches_its_path(oracle, case):
    img, mk, st, envs, expect = W.build_case(case)
    assert img.size <= 83200 and img.ndim == case["ndim"]
    cen = W.census(img, mk, st)
    print(case["id"], [(l["c"], l["voxels"], l["gen0"], l["drained"], l["depth"]) for l in cen["levels"]][:8],
          {name: "".join(k[0] for k in W.chain(cen, env)["kinds"]) for name, env in envs})
    want = oracle.watershed_sk(img, mk, st, 1)
    assert np.array_equal(cen["ref"]["labels"], want), int((cen["ref"]["labels"] != want).sum())
    assert (want != 0).all()  # every voxel is reached
    W.check_expect(case, img, mk, st, cen)
    # the vectorised histograms (all the large case has) against the plain census
    table = W.level_table(img, cen["ref"]["cost"], mk, st)
    assert [{k: l[k] for k in ("c", "voxels", "gen0", "drained")} for l in cen["levels"]] == [{k: l[k] for k in ("c", "voxels", "gen0", "drained")} for l in table]
    if cen["tied"] == 0:  # no tied markers of different labels: the heap's own tie order gives the same flood -- scikit-image's
        assert np.array_equal(oracle.watershed_sk(img, mk, st, 0), want)
    else:  # the one row with tied markers (see the table): the count is the header's, stated plainly
        assert case["id"] == "lattice-overflow"
        lab = mk.ravel()[mk.ravel() != 0]
        assert cen["tied"] == int((lab[1:] != lab[:-1]).sum()) and not img.any()
    for dt in case["mk_dtypes"]:
        assert np.array_equal(mk.astype(dt), mk)


def test_every_path_of_the_issue_has_a_row():
    by = {c["id"]: c for c in W.CASES}
    kinds = lambda cid, name: "".join(by[cid]["expect"]["kinds"][name])
    assert "r" in kinds("corridor-wrap-1", "solo0") and "r" in kinds("corridor-basins", "resident")
    assert all(set(kinds(c, "tile")) == {"t"} for c in by if c.startswith("tile-faces"))
    assert kinds("mixed-chain", "default") == "sstrsss"  # a small run, a tile-wise level, a resident level, a small run
    assert {c["conn"] for c in W.CASES if c["id"].startswith("tile-faces")} == {1, 2, 3}
    assert {(c["ndim"], c["conn"]) for c in W.CASES if c["id"].startswith("small-2d")} == {(2, 1), (2, 2)}
    for c in W.CASES + W.LATE_CASES:
        assert c["envs"][0] == ("default", {}) and len(dict(c["envs"])) == len(c["envs"])


def test_small_switches_sit_on_and_past_the_constants():
    by = {c["id"]: c["expect"] for c in W.CASES}
    assert by["small-gen0-4096"]["gen0"] == W.SMALL_GEN0 and by["small-gen0-4097"]["gen0"] == W.SMALL_GEN0 + 1
    assert by["small-total-32768"]["voxels"] == W.SMALL_TOTAL and by["small-total-32769"]["voxels"] == W.SMALL_TOTAL + 1
    for a, b in (("small-gen0-4096", "small-gen0-4097"), ("small-total-32768", "small-total-32769")):
        assert by[b]["runs"] - by[a]["runs"] == 1  # the level past the switch cuts the run in two


def test_late_record_condition_at_the_chosen_shape():
    """the smallest number of 203 x 237 slices that grants the records; one row of tiles (16 rows, 8 slices) less does not"""
    d, h, w = W.LATE_SHAPE
    assert d % W.TZ and h % W.TY and w % W.TX
    assert W.late_records_granted(d * h * w, 6) and not W.late_records_granted((d - 1) * h * w, 6)
    assert not W.late_records_granted(d * (h - W.TY) * w, 6) and not W.late_records_granted((d - W.TZ) * h * w, 6)
    assert not W.late_records_granted(d * h * w, 26) and not W.late_records_granted(d * h * w, 6, {"IVX_SK_LATE_RECS": "0"})
    assert not W.late_records_granted(d * h * w, 6, {"IVX_SK_SPLIT": "0"})
    assert W.late_records_granted(2 ** 23, 6) and not W.late_records_granted(2949120, 6)  # (40, 192, 384), the largest case there was
    # the arithmetic by hand: 12 000 records of 32 bytes are 384 000 bytes, a multiple of 256
    n = d * h * w
    assert n - n // 8 >= 1024 + 2 * 384000 + 2 ** 22 > (d - 1) * h * w - (d - 1) * h * w // 8


def test_late_record_levels_on_a_small_volume(monkeypatch):
    """late_record_levels on a volume one can count, with the grant's size condition out of the way: three slabs of values
    0 | 4 | 9 along x, 4 x 6 in cross-section, the marker in slab 0.  Level 4's generation 0 is the plane next to slab 0: all its
    lower neighbours lie in level 0, the level right below -- all late, no early part, nothing queued.  Level 9's plane next to
    slab 4 is late in the same way (24 voxels).  One voxel of value 9 in slab 0's corner has its lower neighbours in level 0, not
    in level 4: level 9's early part, but 24 late of 25 is more than half: still nothing.  With the whole plane x = 0 at 9 the
    early part has 24 voxels, the late part 24 of 48: level 9 is queued and gets records."""
    st = generate_binary_structure(3, 1)
    env = {"IVX_SK_SMALL": "0", "IVX_SK_TILE_LEVEL": "0"}
    monkeypatch.setattr(W, "late_records_granted", lambda n, conn, env=None: conn == 6)
    img = np.repeat(np.array([0] * 5 + [4] * 5 + [9] * 5, np.uint16)[None, None], 4, 0).repeat(6, 1)
    mk = np.zeros(img.shape, np.int16)
    mk[2, 3, 2] = 1
    img[0, 0, 0] = 9
    table = W.level_table(img, W.flood(img, mk, st)["cost"], mk, st)
    assert table == [dict(c=0, voxels=119, gen0=1, drained=0, late=0), dict(c=4, voxels=120, gen0=24, drained=0, late=24),
                     dict(c=9, voxels=121, gen0=25, drained=0, late=24)]
    assert W.late_record_levels(table, img.size, 6, env) == []
    img[:, :, 0] = 9
    cost = W.flood(img, mk, st)["cost"]
    assert np.array_equal(cost, img)
    table = W.level_table(img, cost, mk, st)
    assert table[2] == dict(c=9, voxels=144, gen0=48, drained=0, late=24)
    assert W.late_record_levels(table, img.size, 6, env) == [9]
    assert W.late_record_levels(table, img.size, 6, dict(env, IVX_SK_LATE_MAX="23")) == []  # a late part longer than the brute-force limit
    assert W.late_record_levels(table, img.size, 6, {}) == []  # all levels small: nobody takes the stamping path
    assert W.late_record_levels(table, img.size, 26, env) == []  # 26 neighbours: refused
    assert W.chain_of_table(table, env) == dict(kinds=["resident"] * 3, small_level_runs=0, tile=False, resident_levels=3)


def _defines(text, pattern):
    assert re.search(pattern, text), pattern


def test_restated_constants_are_the_files():
    hip = open(os.path.join(HIP, "k_wssk.hip")).read()
    tiles = open(os.path.join(HIP, "ws_tiles.h")).read()
    _defines(hip, r"constexpr int SMALL_GEN0 = %d;" % W.SMALL_GEN0)
    _defines(hip, r"constexpr uint32_t SMALL_TOTAL = %d;" % W.SMALL_TOTAL)
    _defines(hip, r"constexpr int WB_CAP = %d;" % W.WB_CAP)
    _defines(hip, r"constexpr uint32_t SK_SOLO_MAX = %d;" % W.SK_SOLO_MAX)
    _defines(hip, r"constexpr uint32_t PSEQ_MOD = 0x%Xu, PSEQ_DONE = 0x%Xu" % (W.PSEQ_MOD, W.PSEQ_MOD))
    _defines(hip, r"constexpr uint32_t LATE_MAX = %d," % W.LATE_MAX)
    _defines(hip, r"k\.tile_min = tenv \? \(uint64_t\)atoll\(tenv\) : \(\(uint64_t\)1 << 16\);")
    assert W.TILE_LEVEL == 1 << 16
    _defines(hip, r"k\.per_wg = epb && atoi\(epb\) >= 32 \? \(uint32_t\)atoi\(epb\) : %du;" % W.PER_WG)
    _defines(hip, r"k\.solo_max = eso \? \(uint32_t\)atoi\(eso\) : SK_SOLO_MAX;")
    _defines(hip, r"bool is_small\(uint32_t c\) const \{ return k\.small_on && hist\[c\] <= \(uint32_t\)SMALL_GEN0 && lhist\[c\] <= SMALL_TOTAL; \}")
    _defines(hip, r"bool is_tile_level\(uint32_t c\) const \{ return dhist\[c\] == 0 && k\.tile_min && lhist\[c\] >= k\.tile_min; \}")
    _defines(hip, r"if \(x\.is_small\(c\)\) \{ // a run of consecutive small levels")  # asked before is_tile_level
    _defines(hip, r"if \(base \+ n <= WB_CAP\) sg\.n\[wv\] = base \+ n;")
    _defines(hip, r"cv\.rec_off = \(cv\.n / 8 \+ 511\) & ~\(size_t\)255;")
    _defines(hip, r"cv\.late_bytes = \(\(size_t\)k\.late_max \* 32 \+ 255\) & ~\(size_t\)255;")
    _defines(hip, r"cv\.small_ok = k\.small_recs && conn == 6;")
    _defines(hip, r"if \(k\.late_recs && k\.split && conn == 6 && cv\.n >= cv\.n / 8 \+ 1024 \+ 2 \* cv\.late_bytes \+ \(\(size_t\)1 << 22\)\)")
    assert W.LATE_SLACK == 1 << 22
    _defines(hip, r"return small_ok && esum && rec_off \+ \(size_t\)esum \* 32 \+ 2 \* late_bytes \+ 512 <= n \?")
    _defines(hip, r"if \(x\.is_small\(cn\) \|\| x\.is_tile_level\(cn\) \|\| ce == 0 \|\| cl > x\.hist\[cn\] / 2\) return IVX_OK;")
    _defines(hip, r"if \(x\.carve\.late_recs\[set\] && cl && cl <= x\.k\.late_max\)")
    _defines(hip, r"const bool solo = \(nph \? ndl : nfr\) <= solo_max;")
    _defines(hip, r"const uint32_t nactive = min\(n_wg, \(n_in \+ per_wg - 1u\) / per_wg\);")
    _defines(hip, r"if \(m && \(int\)mk\[front\[i - 1\]\] != m\) atomicAdd\(&st->mixed, 1u\);")
    _defines(hip, r"for \(uint32_t c = 0; c < 65535; c\+\+\) \{\n        const uint32_t cnt = x\.hist\[c\], ndl = x\.dhist\[c\];")  # the chain ends below 65535
    _defines(tiles, r"TZ = %d," % W.TZ)
    _defines(tiles + open(os.path.join(HIP, "..", "build.py")).read(), r"IVX_WS_TX\D+%d" % W.TX)


# ---- the reference and the census on volumes one can count by hand ----------------------------------------------------------------
def test_census_of_a_line():
    """I = 3 5 5 2 5 9 0 with markers 1 | 2 at the ends.  Costs 3 5 5 5 5 9 0.  Level 0: the right marker.  Level 3: the left
    marker.  Level 5: generation 0 is voxel 1 alone (next to cost 3; voxel 4's right neighbour costs 9); voxel 2 follows one
    generation later and stamps the basin {3} (value 2 < 5), which relays to voxel 4 one generation after that: depth 2, one
    basin generation (the second of the level).  Level 9: voxel 5, generation 0 from both sides; voxel 4 (level 5, label 1) was
    popped after voxel 6 (level 0), so the smallest time among its lower neighbours is the right marker's: label 2."""
    img = np.array([[[3, 5, 5, 2, 5, 9, 0]]], np.uint16)
    mk = np.array([[[1, 0, 0, 0, 0, 0, 2]]], np.int16)
    st = generate_binary_structure(3, 1)
    cen = W.census(img, mk, st)
    assert cen["ref"]["cost"].ravel().tolist() == [3, 5, 5, 5, 5, 9, 0]
    assert cen["ref"]["labels"].ravel().tolist() == [1, 1, 1, 1, 1, 2, 2]
    assert cen["ref"]["G"].tolist() == [2, 3, 4, 4, 5, 6, 1]
    assert cen["levels"] == [dict(c=0, voxels=1, gen0=1, drained=0, depth=0, fronts=[1], basin_gens=[]),
                             dict(c=3, voxels=1, gen0=1, drained=0, depth=0, fronts=[1], basin_gens=[]),
                             dict(c=5, voxels=4, gen0=1, drained=1, depth=2, fronts=[1, 1, 1], basin_gens=[1]),
                             dict(c=9, voxels=1, gen0=1, drained=0, depth=0, fronts=[1], basin_gens=[])]
    assert cen["generations"] == 7 and cen["generation0"] == 4 and cen["tied"] == 0
    res = W.chain(cen, W.RES)
    # four resident levels: 1 + 1 + (3 A rounds + 1 relay) + 1 rounds that did work, 2 generation steps
    assert (res["frontier_launches"], res["generation_steps"], res["basin_rounds"], res["resident_levels"]) == (7, 2, 1, 4)
    assert res["frontier_launches"] == res["generation_steps"] + res["basin_rounds"] + res["resident_levels"]
    assert W.chain(cen, {})["small_level_runs"] == 1 and W.chain(cen, W.TILE)["kinds"] == ["tile", "tile", "resident", "tile"]


def test_census_of_the_reference_fixture(oracle):
    """the 5x5x5 fixture of the reference's own test: a cube of 100 in a shell of 0, marker 1 in the cube's centre, marker 2 on
    a corner of the shell.  Level 0: the shell from the corner, 12 steps to the opposite corner.  Level 100: the centre marker
    and the cube's 26 other voxels, all of them generation 0 (every one touches the shell)."""
    image = np.zeros((5, 5, 5), np.uint16)
    image[1:4, 1:4, 1:4] = 100
    mk = np.zeros((5, 5, 5), np.int16)
    mk[2, 2, 2], mk[0, 0, 0] = 1, 2
    st = generate_binary_structure(3, 1)
    cen = W.census(image, mk, st)
    assert [(l["c"], l["voxels"], l["gen0"], l["drained"], l["depth"]) for l in cen["levels"]] == [(0, 98, 1, 0, 12), (100, 27, 27, 0, 0)]
    assert cen["generations"] == 15 and cen["generation0"] == 28
    lab = cen["ref"]["labels"]
    assert (lab == 1).sum() == 1 and (lab == 2).sum() == 124 and np.array_equal(lab, oracle.watershed_sk(image, mk, st, 1))


def test_handover_words_and_solo_stretches():
    """fronts 1 300 2 1 with a relay of 400 drained voxels after the second generation"""
    level = dict(fronts=[1, 300, 2, 1], basin_gens=[1], drained=400)
    # rounds: A1 | A300 B400 A2 A1.  Never solo: a word before each of the four later rounds and the one that ends the level
    assert W.handover(level, 0) == (5, 1)
    # solo up to 256: words before A300 and B400 (both too long), then A2 and A1 in one stretch that begins two generations
    assert W.handover(level, 256) == (3, 2)
    assert W.handover(dict(fronts=[1] * 5, basin_gens=[], drained=0), 256) == (1, 4)


def test_first_round_wave_appends_of_a_small_lattice():
    """a flat 7 x 7 x 130 with markers on the lattice: 3 x 3 x 44 = 396 markers, seven waves.  With 26 neighbours a marker inside
    appends 26 voxels and nobody else offers them; a wave of 64 markers is 16 lattice columns of x and a bit, its voxels never
    touch another wave's markers except in the planes between two waves' columns -- which belong to exactly one marker too."""
    img, mk = W.lattice((7, 7, 130), True)
    st = generate_binary_structure(3, 3)
    cen = W.census(img, mk, st)
    waves = W.first_round_wave_appends(img, mk, st, cen, 0)
    assert len(waves) == 7 and sum(waves) == 7 * 7 * 130 - 396 == cen["levels"][0]["fronts"][1]  # every voxel has exactly one marker
    assert max(waves) > W.WB_CAP
    assert max(W.first_round_wave_appends(img, mk, generate_binary_structure(3, 1), W.census(img, mk, generate_binary_structure(3, 1)), 0)) <= 64 * 6
