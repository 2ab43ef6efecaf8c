"""GPU parity: the coarse pass of the region-growing engine (k_flood_block_flags -> k_flood_coarse -> k_flood_block_apply
in csrc/k_flood.hip) at every block width, rows-per-lane count and size limit, bit for bit against the C oracle.

The cases come from tests/_flood_cases.py; tests/test_flood_cases_host.py holds them, on the CPU, against a second
reference (scipy.ndimage.label), against the facts they were built to have, and against ivx_flood_describe for the path
each shape takes.  Bits cannot tell a coarse pass that reaches too little (the rounds complete whatever it leaves), so
where the pass must carry the flood the round count DeviceVolume.region_grow returns is held against the tile distance.

The two quantities that had to be seen on the GPU once (they are asserted as windows / inequalities that follow from the
engine's design, the observed values are for the reader): the 31-tile line of ring_corridor() takes 32 rounds under 6 and
31 under 26 neighbours, and an all-candidate volume takes 0 rounds with the coarse pass on (10 / 18 / 33 without, at 1000 /
2000 / 4000 voxels along x)."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _flood_cases as fc

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


@functools.lru_cache(maxsize=None)
def _reference(kind, key, conn):
    """the oracle's floods of a case, computed once"""
    from oracle import oracle as orc
    orc.build()
    case = getattr(fc, kind)(*key)
    ref = fc.run_floods(case, conn, orc.floodfill_threshold)
    for _, _, before, after in ref:
        before.setflags(write=False)
        after.setflags(write=False)
    return ref


def _check_floods(case, conn, got, ref):
    """same bits as the oracle; per body, filled voxels = all of its candidates or none, as the case was built"""
    for (name, fill, before, after), (_, _, before_r, after_r) in zip(got, ref):
        assert np.array_equal(before, before_r), name
        if case.joined:
            for body, (n, cand) in fc.body_counts(case, fill, before, after).items():
                want = cand if body in case.joined[conn][name] else 0
                assert n == want, "flood %s, conn %d: body %s has %d of %d voxels filled, expected %d" % (name, conn, body, n, cand, want)
        assert np.array_equal(after, after_r), "flood %s, conn %d: %d voxels differ" % (name, conn, int((after != after_r).sum()))


def _grow(case, conn, flood=0):
    """one flood of the case on a resident volume -> (rounds, out)"""
    from invesalius3_amd.device import DeviceVolume
    _, seeds, fill = case.floods[flood]
    with DeviceVolume(np.ascontiguousarray(case.img)) as vol:
        if case.out0.any():
            vol.out_mask.upload(np.ascontiguousarray(case.out0))
        rounds = vol.region_grow(seeds, fc.T0, fc.T1, fc.structure(conn), fill=fill, select_value=None)
        return rounds, vol.download_out_mask()


def _child(code, **env):
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path[:0] = [%r, %r]\n" % (ROOT, TESTS) + code],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child-ok" in r.stdout, r.stdout + r.stderr
    return r


# ---- (a) block widths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [1, 2, 3])
@pytest.mark.parametrize("dx", fc.WIDTHS)
def test_block_widths_join_what_touches(ivxlib, dx, conn):
    """blocks of 16 / 32 / 64 voxels and the pass switched off at 4097: face, edge and corner contacts of whole blocks,
    a block one voxel short, a missing block and a missing plane, the last partial word; fused and unfused starts, and a
    second fill value into the same out array"""
    from invesalius3_amd import invesalius_rs as floodfill
    case = fc.widths_case(dx)
    _check_floods(case, conn, fc.run_floods(case, conn, floodfill.floodfill_threshold), _reference("widths_case", (dx,), conn))


# ---- (b) forced blocks and switches -----------------------------------------------------------------------------------------
SWITCH_CODE = (
    "import numpy as np\n"
    "import _flood_cases as fc\n"
    "from conftest import synth_volume\n"
    "from invesalius3_amd import invesalius_rs as ff\n"
    "from oracle import oracle as orc\n"
    "img = synth_volume((40, 72, 136), seed=91)\n"
    "z, y, x = np.unravel_index(np.argmax(img), img.shape)\n"
    "seeds = [(int(x), int(y), int(z)), (5, 5, 5)]\n"
    "case = fc.widths_case(1100)\n"
    "for conn in (1, 2, 3):\n"
    "    s = fc.structure(conn)\n"
    "    og0 = (np.random.default_rng(3 + conn).random(img.shape) < 0.02).astype(np.uint8); og = og0.copy(); orf = og0.copy()\n"
    "    ff.floodfill_threshold(img, seeds, -820, 3071, 1, s, og)\n"
    "    orc.floodfill_threshold(img, seeds, -820, 3071, 1, s, orf)\n"
    "    assert np.array_equal(og, orf), ('phantom', conn)\n"
    "    assert 64 * 16 * 16 < int((orf == 1).sum()) - int((og0 == 1).sum()) < img.size, conn\n"
    "    got = fc.run_floods(case, conn, ff.floodfill_threshold)\n"
    "    ref = fc.run_floods(case, conn, orc.floodfill_threshold)\n"
    "    for (name, fill, _, a), (_, _, _, b) in zip(got, ref):\n"
    "        assert np.array_equal(a, b), ('1100', name, conn, int((a != b).sum()))\n"
    "print('child-ok')\n")


@pytest.mark.parametrize("switch", ["IVX_FLOOD_BLOCK=32", "IVX_FLOOD_BLOCK=64", "IVX_FLOOD_COARSE=0", "IVX_FLOOD_FUSED=0"])
def test_forced_blocks_and_switches(ivxlib, oracle, switch):
    """the switches are read once per process: a fresh one per setting, the 3-D phantom of test_all_flood_engines_agree
    (block 16 by itself) and the 1100 wide case (block 32 by itself), under the three standard structures"""
    name, value = switch.split("=")
    _child(SWITCH_CODE, **{name: value})


# ---- (c) rows per lane and the LDS limit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [1, 3])
@pytest.mark.parametrize("name", list(fc.ROWS))
def test_rows_per_lane_and_lds_limit(ivxlib, name, conn):
    """65 rows of tiles (128 lanes), 1025 (the first second slot), 86 x 85 (eight rows in every lane, the last grid that
    fits) and 86 x 86 (the pass is off: clear + seed + build_list, then the escape to the union-find engine).  A round
    moves the flood one tile at most, so without the coarse pass the slab costs at least hops26 rounds (or the escape at
    48); with it, fewer: that is what says the fix-point carried across the row slots."""
    from invesalius3_amd import invesalius_rs as floodfill
    case = fc.rows_case(name)
    ref = _reference("rows_case", (name,), conn)
    _check_floods(case, conn, fc.run_floods(case, conn, floodfill.floodfill_threshold), ref)
    rounds, out = _grow(case, conn)
    print("rounds", name, conn, rounds)
    assert np.array_equal(out, ref[0][3])
    hops = case.facts["hops26"]
    if name == "rows86x86":
        assert rounds >= min(hops, fc.ESCAPE)
    else:
        assert rounds < min(hops, fc.ESCAPE)


# ---- (d) tile-level serpentine, all-candidate volumes -----------------------------------------------------------------------
ROUNDS_CODE = (
    "import json, numpy as np\n"
    "import _flood_cases as fc\n"
    "from invesalius3_amd.device import DeviceVolume\n"
    "from oracle import oracle as orc\n"
    "res = {}\n"
    "for key, case in [('snake', fc.tile_serpentine())] + [('all%d' % dx, fc.all_candidate(dx)) for dx in fc.ALL_CANDIDATE_WIDTHS]:\n"
    "    (_, seeds, fill), = case.floods\n"
    "    (_, _, _, ref), = fc.run_floods(case, 1, orc.floodfill_threshold)\n"
    "    with DeviceVolume(np.ascontiguousarray(case.img)) as vol:\n"
    "        res[key] = vol.region_grow(seeds, fc.T0, fc.T1, fc.structure(1), fill=fill, select_value=None)\n"
    "        assert np.array_equal(vol.download_out_mask(), ref), key\n"
    "print('rounds=' + json.dumps(res))\n"
    "print('child-ok')\n")


@pytest.fixture(scope="module")
def rounds_without_coarse(ivxlib, oracle):
    r = _child(ROUNDS_CODE, IVX_FLOOD_COARSE="0")
    return json.loads(re.search(r"rounds=(\{.*\})", r.stdout).group(1))


def test_tile_serpentine_is_crossed_by_the_coarse_pass(ivxlib, rounds_without_coarse):
    """568 tile hops of whole tiles: the coarse pass takes them all, the rounds alone give up at 48 and escape"""
    case = fc.tile_serpentine()
    (_, _, _, ref), = _reference("tile_serpentine", (), 1)
    rounds, out = _grow(case, 1)
    print("rounds snake", rounds, "without coarse", rounds_without_coarse["snake"])
    assert np.array_equal(out, ref)
    assert rounds < fc.ESCAPE
    assert rounds_without_coarse["snake"] >= fc.ESCAPE


@pytest.mark.parametrize("dx", fc.ALL_CANDIDATE_WIDTHS)
def test_all_candidate_volume_needs_no_round(ivxlib, rounds_without_coarse, dx):
    """every existing block is wholly reached, so k_flood_block_apply enlists nothing: 0 rounds (seen on the GPU at the
    three block widths), against one round per tile between the seed and the far end without the pass"""
    case = fc.all_candidate(dx)
    (_, _, _, ref), = _reference("all_candidate", (dx,), 1)
    rounds, out = _grow(case, 1)
    off = rounds_without_coarse["all%d" % dx]
    print("rounds all-candidate", dx, rounds, "without coarse", off)
    assert np.array_equal(out, ref)
    assert rounds < off
    assert rounds == 0


# ---- (e) lists longer than the grid, many seeds, ring wrap ------------------------------------------------------------------
@pytest.mark.parametrize("conn", [1, 3])
def test_list_longer_than_the_grid(ivxlib, conn):
    """2600 tiles on the first round's list against a grid of 1536 workgroups: the workgroups stride over the list; 5000
    seeds leave the fused start and take two staging chunks"""
    from invesalius3_amd import invesalius_rs as floodfill
    case = fc.long_list()
    _check_floods(case, conn, fc.run_floods(case, conn, floodfill.floodfill_threshold), _reference("long_list", (), conn))


TRACE_CODE = (
    "import numpy as np\n"
    "import _flood_cases as fc\n"
    "from invesalius3_amd import invesalius_rs as ff\n"
    "from oracle import oracle as orc\n"
    "case = fc.long_list()\n"
    "got = fc.run_floods(case, 1, ff.floodfill_threshold)\n"
    "ref = fc.run_floods(case, 1, orc.floodfill_threshold)\n"
    "assert np.array_equal(got[0][3], ref[0][3])\n"
    "print('child-ok')\n")


def test_first_round_reports_a_list_longer_than_the_grid(ivxlib, oracle):
    case = fc.long_list()
    woken = fc.woken_tiles(case)
    assert woken > fc.GRID_CAP
    r = _child(TRACE_CODE, IVX_FLOOD_TRACE="1")
    lines = re.findall(r"ivx flood: round (\d+) starts with (\d+) of (\d+) tiles", r.stderr)
    assert lines, r.stderr
    print("trace", lines[:4])
    first_round, n_list, ntiles = (int(v) for v in lines[0])
    assert ntiles == 2600 and n_list > fc.GRID_CAP
    if first_round == 1:
        assert n_list == woken


@pytest.mark.parametrize("conn", [1, 3])
def test_counter_ring_wraps_below_the_escape(ivxlib, conn):
    """a voxel-wide line through 31 tiles: one round per tile (32 / 31 seen on the GPU under 6 / 26 neighbours), past the 16 entries of the counter
    ring and short of the escape at 48"""
    case = fc.ring_corridor()
    (_, _, _, ref), = _reference("ring_corridor", (), conn)
    rounds, out = _grow(case, conn)
    print("rounds ring", conn, rounds)
    assert np.array_equal(out, ref)
    assert fc.RING < rounds < fc.ESCAPE
