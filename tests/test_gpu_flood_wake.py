"""The wake-up rule of the region-growing rounds (csrc/k_flood.hip, tile_update): a visit wakes a neighbour tile only for an
open candidate -- a voxel of that tile in the visit's staged halo that is a candidate, was unreached, and lies in the 3 x 3 x 3
neighbourhood of one of the visit's new bits.  A wake-up too few leaves candidates unreached, so every case compares the
reached bytes and the mask with the CPU oracle (labelling, or propagation for the structuring element that is not
symmetric); a wake-up too many only costs time, so (c) and (d) also hold the visit and round counts
(ivx_dev_flood_visits) against the rule restated in numpy.  Volumes are 3 x 3 x 3 tiles; cases in _flood_wake_cases.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _flood_wake_cases as wc

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
STRUCTURES = {"26": wc.fc.structure(3), "18": wc.fc.structure(2), "6": wc.fc.structure(1), "asym": wc.asym_structure()}


@functools.lru_cache(maxsize=None)
def _reference(kind, key, sname):
    """the oracle's out array of a case's flood, computed once"""
    case = getattr(wc, kind)(*key)
    (_, seeds, fill), = case.floods
    out = case.out0.copy()
    if sname == "asym":
        wc.propagate_flood(case.img, seeds, fill, STRUCTURES[sname], out)
    else:
        wc.label_flood(case.img, seeds, fill, {"6": 1, "18": 2, "26": 3}[sname], out)
    out.setflags(write=False)
    return out


def _grow(case, strct, repeat=1):
    """threshold + region growing of the case on a resident volume, `repeat` times over:
    [(rounds, visits, first list, out bytes, mask bytes)]"""
    from invesalius3_amd.device import DeviceVolume
    (_, seeds, fill), = case.floods
    res = []
    with DeviceVolume(np.ascontiguousarray(case.img)) as vol:
        for _ in range(repeat):
            vol.zero_out_mask()
            vol.threshold(wc.T0, wc.T1, preserve=False)
            rounds = vol.region_grow(seeds, wc.T0, wc.T1, strct, fill=fill, select_value=254)
            visits, first = vol.flood_visits()
            res.append((rounds, visits, first, vol.download_out_mask(), vol.download_mask()))
    return res


def _check_bits(case, out, mask, ref, what):
    inr = (case.img >= wc.T0) & (case.img <= wc.T1)
    assert np.array_equal(out, ref), "%s: %d reached bytes differ from the oracle" % (what, int((out != ref).sum()))
    want = np.where(ref != 0, 254, np.where(inr, 255, 0)).astype(np.uint8)
    assert np.array_equal(mask, want), "%s: %d mask bytes differ" % (what, int((mask != want).sum()))


# ---- (a) all 26 directions must wake ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sname", ["26", "18", "6", "asym"])
def test_every_direction_wakes(ivxlib, sname):
    """the body of the centre tile touches one candidate of each of the 26 neighbour tiles -- face, edge and corner
    contacts, the pure +-x ones at bits 63 and 0 -- and each carries a tail; under 6 and 18 neighbours (and for the steps
    the asymmetric element lacks) the diagonal contacts do not connect, which the oracle says too"""
    case = wc.contacts_case()
    ref = _reference("contacts_case", (), sname)
    (rounds, visits, first, out, mask), = _grow(case, STRUCTURES[sname])
    print("contacts", sname, "rounds", rounds, "visits", visits, "first list", first)
    _check_bits(case, out, mask, ref, "contacts " + sname)
    for d, ok in wc.contacts_reached(case, STRUCTURES[sname]).items():
        assert bool(out[case.facts["contacts"][d][0]]) == ok, (sname, d)


# ---- (b) a stale halo -------------------------------------------------------------------------------------------------------
def test_stale_halo_whichever_tile_stages_first(ivxlib):
    """two seeded bodies in neighbouring tiles of the first list, parts of each reachable only through the other: the same
    bits from five floods in one process, whichever visit staged its halo first"""
    case = wc.stale_halo_case()
    ref = _reference("stale_halo_case", (), "26")
    assert all(ref[v].all() for v in case.bodies.values())
    for n, (rounds, visits, first, out, mask) in enumerate(_grow(case, STRUCTURES["26"], repeat=5)):
        print("stale halo run", n, "rounds", rounds, "visits", visits, "first list", first)
        _check_bits(case, out, mask, ref, "stale halo, run %d" % n)


# ---- (c) wake-ups that must not happen --------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [1, 0])
def test_no_wake_without_an_open_candidate(ivxlib, axis):
    """the seeded body changes the whole face towards the next tile of the line, whose nearest candidate is two voxels
    away: nobody is woken, the first list is all there is.  (The rule before this one -- wake every tile that can see a
    changed face -- visits the next tile once more: model_rounds(..., "faces") gives 2 rounds and 28 visits for a first
    list of 27.)"""
    case = wc.no_wake_case(axis)
    ref = _reference("no_wake_case", (axis,), "26")
    (_, seeds, _), = case.floods
    m_rounds, m_visits, m_first, m_reached = wc.model_rounds(case.img, seeds, "open")
    assert np.array_equal(m_reached, ref != 0) and (m_rounds, m_visits) == (1, m_first)
    (rounds, visits, first, out, mask), = _grow(case, STRUCTURES["26"])
    print("no wake, axis", axis, "rounds", rounds, "visits", visits, "first list", first, "model", (m_rounds, m_visits, m_first))
    _check_bits(case, out, mask, ref, "no wake")
    assert first == m_first
    assert visits == first
    assert rounds == 1


# ---- (d) a single chain -------------------------------------------------------------------------------------------------------
def test_chain_visits_one_tile_per_round(ivxlib):
    """a snake through nine tiles: one round per tile of the chain -- rounds equal the tile distance from the seed's tile
    plus one -- and after the first list one visit per round.  (Not _flood_cases.tile_serpentine(): its corridors are whole
    tiles, which the coarse pass crosses without a round, and with the pass switched off its 568 tile hops end in the
    union-find escape at 48 rounds, so neither gives a round or a visit count to hold; chain_case() is the same shape in
    voxel-wide lines that no block can swallow, and its docstring says why the count is deterministic.)"""
    case = wc.chain_case()
    ref = _reference("chain_case", (), "26")
    (_, seeds, _), = case.floods
    m_rounds, m_visits, m_first, m_reached = wc.model_rounds(case.img, seeds, "open")
    assert np.array_equal(m_reached, ref != 0)
    assert m_rounds == case.facts["tiles"] and m_visits == m_first + case.facts["tiles"] - 1
    (rounds, visits, first, out, mask), = _grow(case, STRUCTURES["26"])
    print("chain rounds", rounds, "visits", visits, "first list", first, "model", (m_rounds, m_visits, m_first))
    _check_bits(case, out, mask, ref, "chain")
    assert rounds == m_rounds
    assert first == m_first
    assert visits == m_visits


# ---- (e) the iteration cap ------------------------------------------------------------------------------------------------------
ITCAP_CODE = (
    "import numpy as np\n"
    "import _flood_wake_cases as wc\n"
    "from invesalius3_amd.device import DeviceVolume\n"
    "case = wc.contacts_case()\n"
    "(_, seeds, fill), = case.floods\n"
    "for conn in (3, 1):\n"
    "    ref = case.out0.copy()\n"
    "    wc.label_flood(case.img, seeds, fill, conn, ref)\n"
    "    with DeviceVolume(np.ascontiguousarray(case.img)) as vol:\n"
    "        vol.threshold(wc.T0, wc.T1, preserve=False)\n"
    "        rounds = vol.region_grow(seeds, wc.T0, wc.T1, wc.fc.structure(conn), fill=fill, select_value=254)\n"
    "        out, mask = vol.download_out_mask(), vol.download_mask()\n"
    "    print('itcap 2, conn', conn, 'rounds', rounds)\n"
    "    assert rounds > 4, rounds\n"
    "    assert np.array_equal(out, ref), (conn, int((out != ref).sum()))\n"
    "    inr = (case.img >= wc.T0) & (case.img <= wc.T1)\n"
    "    assert np.array_equal(mask, np.where(ref != 0, 254, np.where(inr, 255, 0)).astype(np.uint8)), conn\n"
    "print('child-ok')\n")


def test_iteration_cap_revisits_the_tile(ivxlib):
    """IVX_FLOOD_ITCAP=2 (read once per process: a child): the body needs ten rows from the seed to its far faces, so the
    centre tile re-enlists itself round after round (more than four rounds) and still wakes all its neighbours"""
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path[:0] = [%r, %r]\n" % (ROOT, TESTS) + ITCAP_CODE],
                       env=dict(os.environ, IVX_FLOOD_ITCAP="2"), capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "child-ok" in r.stdout, r.stdout + r.stderr


# ---- (f) a partial tile ---------------------------------------------------------------------------------------------------------
PARTIAL = ((40, 40, 100), (1, 1, 0))


@pytest.mark.parametrize("sname", ["26", "6", "asym"])
def test_partial_tiles_and_last_word(ivxlib, sname):
    """dx = 100 (the last word holds 36 voxels), 40 rows and slices (the last tiles hold 8): the body's contacts towards
    +y, +z and +x lie in partial tiles, the -x ones do not exist"""
    case = wc.contacts_case(*PARTIAL)
    assert len(case.facts["contacts"]) == 17 and (1, 1, 1) in case.facts["contacts"]
    ref = _reference("contacts_case", PARTIAL, sname)
    (rounds, visits, first, out, mask), = _grow(case, STRUCTURES[sname])
    print("partial", sname, "rounds", rounds, "visits", visits, "first list", first)
    _check_bits(case, out, mask, ref, "partial " + sname)
    for d, ok in wc.contacts_reached(case, STRUCTURES[sname]).items():
        assert bool(out[case.facts["contacts"][d][0]]) == ok, (sname, d)
