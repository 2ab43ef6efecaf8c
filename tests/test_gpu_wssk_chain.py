"""The level chain of the GUI-default watershed (csrc/k_wssk.hip, stage 3) on the cases of _wssk_cases.py, each built for one
path of the chain (test_wssk_cases_host.py proves on the CPU that it gets there): the resident launch with the control word's
sequence number wrapping, with solo stretches of more than a thousand generations, with basin relays that leave a solo stretch;
a wave's staging buffer overflowing; the tile-wise relaxation at partial tiles, with generation 0 on tile faces and plateaus in
parts; runs of small levels on and past their two switches, with and without key records; a chain that goes small run ->
tile-wise -> resident -> small run up to level 65534; late-part key records at the size that grants them.

Everything is integer and exact: labels against the serial oracle and the plain reference, the cost map against the reference's,
and the call's statistics against the census -- generations and generation 0 are the same on every path, which is what catches a
hand-over that loses or doubles a generation without changing a label; the path counters say that the path was taken."""
import warnings

import numpy as np
import pytest

import _wssk_cases as W

pytestmark = pytest.mark.gpu

KNOBS = ("IVX_SK_SMALL", "IVX_SK_TILE_LEVEL", "IVX_SK_SOLO", "IVX_SK_PER_WG", "IVX_SK_RES_PER_CU", "IVX_SK_PLANE", "IVX_SK_SMALL_RECS",
         "IVX_SK_LATE_RECS", "IVX_SK_LATE_MAX", "IVX_SK_SPLIT", "IVX_SK_CHUNK", "IVX_SK_SORT", "IVX_SK_LEVELS", "IVX_WS_TRACE")
_BY_ID = {c["id"]: c for c in W.CASES + W.LATE_CASES}
_REF, _GOT, _TABLE = {}, {}, {}
# the same counters whatever the path
SAME = ("generations", "generation0", "tied_markers_of_different_labels", "levels", "markers")


def _rows(cases):
    return [(c["id"], name, dt) for c in cases for dt in c["mk_dtypes"] for name, _ in c["envs"]]


def _ids(rows):
    return ["%s-%s%s" % (cid, name, "" if dt is np.int16 else "-int8") for cid, name, dt in rows]


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def _ref(oracle, cid):
    """(image, markers, structure, the oracle's labels, census or None), computed once per case"""
    if cid not in _REF:
        case = _BY_ID[cid]
        img, mk, st, _, _ = W.build_case(case)
        want = oracle.watershed_sk(img, mk, st, 1)
        cen = W.census(img, mk, st) if case["plain"] else None
        _REF[cid] = _frozen(img, mk, st, want) + (cen,)
    return _REF[cid]


def _flood(oracle, monkeypatch, cid, name, dt):
    """(labels, cost, stats) of the GPU flood under the variant's environment, run once"""
    if (cid, name, dt) not in _GOT:
        from invesalius3_amd import watershed_process as wp
        img, mk, st = _ref(oracle, cid)[:3]
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in dict(_BY_ID[cid]["envs"])[name].items():
            monkeypatch.setenv(k, v)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (the tied-marker warning of the one row that has tied markers)
            _GOT[cid, name, dt] = wp.watershed(img, mk.astype(dt), st, want_cost=True, want_stats=True)
    return _GOT[cid, name, dt]


ROWS = _rows(W.CASES)


@pytest.mark.parametrize("cid,name,dt", ROWS, ids=_ids(ROWS))
def test_chain_case(ivxlib, oracle, monkeypatch, cid, name, dt):
    img, mk, st, want, cen = _ref(oracle, cid)
    env = dict(_BY_ID[cid]["envs"])[name]
    got, cost, stats = _flood(oracle, monkeypatch, cid, name, dt)
    ch = W.chain(cen, env)
    print(cid, name, "".join(k[0] for k in ch["kinds"]), {k: v for k, v in stats.items() if not k.startswith("us_")},
          {k: v for k, v in ch.items() if k != "kinds"})
    assert got.dtype == np.int32 and cost.dtype == np.uint16
    assert np.array_equal(cost, cen["ref"]["cost"]), "cost map: %d voxels differ" % int((cost != cen["ref"]["cost"]).sum())
    assert np.array_equal(got, want), "labels: %d voxels differ from the serial flood" % int((got != want).sum())
    assert np.array_equal(got, cen["ref"]["labels"])
    # the same on every path
    assert stats["generations"] == cen["generations"]
    assert stats["generation0"] == cen["generation0"]
    assert stats["tied_markers_of_different_labels"] == cen["tied"] == _BY_ID[cid]["expect"].get("tied", 0)
    assert stats["levels"] == len(cen["levels"]) and stats["markers"] == int((mk != 0).sum())
    # the path
    assert (stats["tile_rounds"] > 0) == ch["tile"]
    assert stats["small_level_runs"] == ch["small_level_runs"]
    # the resident launches' counters (small runs and tile-wise levels leave them alone): a resident level of depth D with B basin
    # generations closes D + 1 frontier rounds and B relays, and begins D generations after its first -- so the header's "rounds
    # that did work" are generation steps + basin rounds + one per resident level
    assert stats["basin_rounds"] == ch["basin_rounds"]
    assert stats["generation_steps"] == ch["generation_steps"]
    assert stats["frontier_launches"] == ch["frontier_launches"] == ch["generation_steps"] + ch["basin_rounds"] + ch["resident_levels"]
    if _BY_ID[cid]["expect"].get("no_basins"):
        assert stats["basin_rounds"] == 0


@pytest.mark.parametrize("cid,name,dt", ROWS, ids=_ids(ROWS))
def test_variant_equals_the_default_run(ivxlib, oracle, monkeypatch, cid, name, dt):
    a, acost, ast = _flood(oracle, monkeypatch, cid, "default", np.int16)
    b, bcost, bst = _flood(oracle, monkeypatch, cid, name, dt)
    assert np.array_equal(a, b) and np.array_equal(acost, bcost)
    for k in SAME:
        assert ast[k] == bst[k], (k, ast[k], bst[k])


def test_small_run_count_changes_by_one_across_each_switch(ivxlib, oracle, monkeypatch):
    runs = {cid: _flood(oracle, monkeypatch, cid, "default", np.int16)[2]["small_level_runs"]
            for cid in ("small-gen0-4096", "small-gen0-4097", "small-total-32768", "small-total-32769")}
    assert runs == {"small-gen0-4096": 1, "small-gen0-4097": 2, "small-total-32768": 1, "small-total-32769": 2}


def _cost_is_a_fixed_point(img, mk, st, cost):
    """C = I on the markers, C = max(I, smallest C among the neighbours) elsewhere: what every minimax cost map satisfies"""
    d, h, w = img.shape
    Cp = np.full((d + 2, h + 2, w + 2), 65535, np.uint16)
    Cp[1:-1, 1:-1, 1:-1] = cost
    low = np.full(img.shape, 65535, np.uint16)
    for dz, dy, dx in W._offsets3(st):
        np.minimum(low, Cp[1 + dz:1 + dz + d, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w], out=low)
    return np.array_equal(cost, np.where(mk != 0, img, np.maximum(img, low)))


LATE_ROWS = _rows(W.LATE_CASES)


@pytest.mark.parametrize("cid,name,dt", LATE_ROWS, ids=_ids(LATE_ROWS))
def test_late_record_case(ivxlib, oracle, monkeypatch, cid, name, dt):
    """5.7 M voxels, the one case without a plain reference (it would take minutes; the serial oracle takes two seconds, once per
    structure): labels against the oracle, the cost map as a fixed point of its rule, the chain's histograms from the cost map
    (level_table, which the host test checks against the plain census on every small case), and every variant's path-
    independent counters against the default run's."""
    img, mk, st, want, _ = _ref(oracle, cid)
    case = _BY_ID[cid]
    env = dict(case["envs"])[name]
    got, cost, stats = _flood(oracle, monkeypatch, cid, name, dt)
    assert np.array_equal(got, want), "labels: %d voxels differ from the serial flood" % int((got != want).sum())
    if cid not in _TABLE:
        assert _cost_is_a_fixed_point(img, mk, st, cost)
        _TABLE[cid] = W.level_table(img, cost, mk, st)
    table = _TABLE[cid]
    ch = W.chain_of_table(table, env)
    recs = W.late_record_levels(table, img.size, int(st.sum()) - 1, env)
    print(cid, name, {k: v for k, v in stats.items() if not k.startswith("us_")}, "levels keyed from records:", len(recs),
          "kinds:", {k: ch["kinds"].count(k) for k in ("small", "tile", "resident")})
    dcost, dstats = _flood(oracle, monkeypatch, cid, "default", dt)[1:]
    assert np.array_equal(cost, dcost)
    for k in SAME:
        assert stats[k] == dstats[k], (k, stats[k], dstats[k])
    assert stats["tied_markers_of_different_labels"] == W.tied_markers(img, mk) == 0
    assert stats["generation0"] == sum(l["gen0"] for l in table) and stats["levels"] == len(table)
    assert table[0]["c"] == 0 and ch["kinds"][0] == "tile" and stats["tile_rounds"] > 0  # the zero plateau
    assert stats["small_level_runs"] == ch["small_level_runs"]
    assert stats["frontier_launches"] == stats["generation_steps"] + stats["basin_rounds"] + ch["resident_levels"]
    # the records: granted at 6 neighbours and this size, used where every level takes the stamping path
    assert W.late_records_granted(img.size, 6) and (len(recs) > 0) == (cid == "late-records-6" and name == "resident")
