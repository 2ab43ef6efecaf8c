"""The run-based union-find of csrc/k_ccl.hip past one tile (8 words x 8 rows x 4 slices), one word and one scan block
(4096 words): Mask.fill_holes_auto, which always goes through it, and the region grows that take it (IVX_FLOOD_MODE=ccl,
the escape after 48 frontier rounds, from the host mirror and from DeviceVolume.region_grow).  Every input is 1030 or 1100 voxels wide -- three
tiles along x, a partial last word -- and comes from tests/_ccl_ref.py, whose cases tests/test_ccl_cases_host.py checks
on the host.  The results are integers: every comparison is bit for bit, against the numpy / scipy recipe of
_ccl_ref.py AND the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.ndimage import generate_binary_structure

import _ccl_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _both_references(oracle, m, target, conn, orientation, index, size):
    want, ret = R.fill_holes(m, target, conn, orientation, index, size)
    orc = m.copy()
    ret0 = oracle.mask_fill_holes_auto(orc, target, conn, orientation, index, size)
    assert ret == ret0 and np.array_equal(want, orc)  # the two references say the same (also checked on the host)
    return want, ret


@pytest.mark.parametrize("conn", [6, 18, 26])
@pytest.mark.parametrize("case", R.CASES)
def test_fill_holes_3d_across_tiles_words_and_scan_blocks(ivxlib, oracle, case, conn):
    """A noise: every tile boundary, two scan blocks, sizes 5 | 6 at the rule's edge; B checker: 32 runs per word, 8192
    nodes per tile, label 0 at exactly `size`; C solid: runs that continue through every word and tile boundary; D
    stairs: the diagonal contacts bit 63 <-> bit 0 inside and across tiles; E edges: bars in the partial last word and
    across the tile boundaries, sizes at and one below each bar's length"""
    from invesalius3_amd import mask as msk
    p = R.pattern(case, conn)
    m = R.mask_of(p)
    groups = R.known_groups(case, conn)
    for size in R.fill_sizes(case, conn):
        want, ret0 = _both_references(oracle, m, "3D", conn, "AXIAL", 0, size)
        got = m.copy()
        ret = msk.fill_holes_auto(got, "3D", conn, "AXIAL", 0, size)
        assert ret is ret0, (size, ret, ret0)
        diff = np.argwhere(got != want)
        assert len(diff) == 0, (size, len(diff), diff[:8].tolist())
        assert not got[0].any() and not got[:, 0].any() and not got[:, :, 0].any()  # the padding planes
        if groups is not None:  # and what the components, as they were built, say without any labelling
            inner, ret1 = R.fill_holes_known(p, groups, size)
            assert ret is ret1 and np.array_equal(got[1:, 1:, 1:], inner), size


@pytest.mark.parametrize("orientation", ["AXIAL", "CORONAL", "SAGITAL"])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("case", ["noise", "stairs"])
def test_fill_holes_2d_paths_across_tiles(ivxlib, oracle, case, conn, orientation):
    """CORONAL is a strided (1, dz, 1030) view and AXIAL (1, dy, 1030), three tiles along x each; SAGITAL (1, dz, dy)"""
    from invesalius3_amd import mask as msk
    m = R.mask_of(R.pattern_2d(case, conn))
    changed = 0
    for index in R.indices_2d(case, orientation):
        for size in R.sizes_2d(case):
            want, ret0 = _both_references(oracle, m, "2D", conn, orientation, index, size)
            got = m.copy()
            ret = msk.fill_holes_auto(got, "2D", conn, orientation, index, size)
            assert ret is ret0, (index, size)
            diff = np.argwhere(got != want)
            assert len(diff) == 0, (index, size, len(diff), diff[:8].tolist())
            changed += ret
    assert changed


def _serpentine_flood(floodfill, oracle, data, conn, fill):
    strct = generate_binary_structure(3, conn)
    og, orf = np.zeros(data.shape, np.uint8), np.zeros(data.shape, np.uint8)
    floodfill.floodfill_threshold(data, [(0, 0, 1)], 0, 127, fill, strct, og)
    oracle.floodfill_threshold(np.ascontiguousarray(data), [(0, 0, 1)], 0, 127, fill, strct, orf)
    return og, orf


@pytest.mark.parametrize("conn", [1, 3])
def test_long_corridor_across_the_x_tiles_escapes_to_union_find(ivxlib, oracle, conn):
    """default engine: the frontier hands over after 48 rounds, on a plane with three union-find tiles along x"""
    from invesalius3_amd import invesalius_rs as floodfill
    img = R.serpentine()
    strct = generate_binary_structure(3, conn)
    og, orf = np.zeros(img.shape, np.uint8), np.zeros(img.shape, np.uint8)
    floodfill.floodfill_threshold(img, [(0, 0, 1)], 1, 1, 9, strct, og)
    oracle.floodfill_threshold(img, [(0, 0, 1)], 1, 1, 9, strct, orf)
    assert np.array_equal(og, orf)
    assert (og[1] == 9).sum() == 30 * 1100 + 30
    specks, joined = int((img[2] == 1).sum()), int((og[2] == 9).sum())  # over a corridor row, or diagonal to one
    assert (0 < joined < specks) if conn == 1 else joined == specks


def test_tables_are_rebuilt_between_a_flood_and_fill_holes(ivxlib, oracle):
    """one process, one mask matrix: a flood that ends in the union-find, fill_holes_auto (same workspaces, the per-run
    flags with another meaning, sizes behind them), then the flood again -- on a matrix whose candidate plane changed"""
    from invesalius3_amd import invesalius_rs as floodfill
    from invesalius3_amd import mask as msk
    p = np.zeros((5, 60, 1100), bool)
    p[:3] = R.serpentine() == 1
    p[4, 30, 1:6] = True   # two holes of 5 and 1 voxels, an empty slice away from the corridor and its specks
    p[4, 40, 600] = True
    m = R.mask_of(p)
    view = m[1:, 1:, 1:]
    for conn, c3 in ((1, 6), (3, 26)):
        before = m.copy()
        og, orf = _serpentine_flood(floodfill, oracle, view, conn, 3)
        assert np.array_equal(og, orf) and (og == 3).sum() > 30 * 1100 and np.array_equal(m, before)
        want, ret0 = _both_references(oracle, m, "3D", c3, "AXIAL", 0, 5)
        ret = msk.fill_holes_auto(m, "3D", c3, "AXIAL", 0, 5)
        assert ret is ret0 is True and np.array_equal(m, want)
        assert (m[5] == 254).sum() == 6 and (m[2] == 254).sum() == 0  # the holes, not the corridor
        og2, orf2 = _serpentine_flood(floodfill, oracle, view, conn, 3)
        assert np.array_equal(og2, orf2) and np.array_equal(og2, og)  # what was filled never belonged to the corridor
        m[...] = before


_CHILD_HEAD = (
    "import sys, numpy as np\n"
    "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "from scipy.ndimage import generate_binary_structure\n"
    "import _ccl_ref as R\n"
    "from oracle import oracle as orc\n") % (os.path.dirname(HERE), HERE)

_CCL_CHILD = _CHILD_HEAD + (
    "from invesalius3_amd import invesalius_rs as ff\n"
    "def flood(img, seeds, strct, out0):\n"
    "    og, orf = out0.copy(), out0.copy()\n"
    "    ff.floodfill_threshold(img, seeds, 50, 150, 1, strct, og)\n"
    "    orc.floodfill_threshold(img, seeds, 50, 150, 1, strct, orf)\n"
    "    assert np.array_equal(og, orf), np.argwhere(og != orf)[:8].tolist()\n"
    "    return og\n"
    "for case in R.CASES:\n"
    "    for conn, c3 in ((1, 6), (2, 18), (3, 26)):\n"
    "        p = R.pattern(case, c3)\n"
    "        img = p.astype(np.int16) * 100\n"
    "        s = generate_binary_structure(3, conn)\n"
    "        seeds = R.flood_seeds(p, c3)\n"
    "        out0 = R.flood_barriers(p.shape, conn)\n"
    "        og = flood(img, seeds, s, out0)\n"
    "        assert (og != out0).any(), (case, conn)\n"
    "        if case == 'noise':\n"
    "            assert np.array_equal(og, R.flood_by_label(p, seeds, 1, s, out0)), conn\n"
    # a point-symmetric element with both x neighbours that is none of 6 / 18 / 26: the centre row and two corners
    "p = R.stairs()\n"
    "img = p.astype(np.int16) * 100\n"
    "s = np.zeros((3, 3, 3), np.uint8); s[1, 1, :] = 1; s[0, 0, 0] = s[2, 2, 2] = 1\n"
    "chains = R.stairs_chains()\n"
    "og = flood(img, [(int(v[0, 2]), int(v[0, 1]), int(v[0, 0])) for _, v in chains], s, np.zeros(p.shape, np.uint8))\n"
    "joined = 0\n"
    "for kind, v in chains:\n"
    "    up = kind == 'zyx' and tuple(v[1] - v[0]) == (1, 1, 1)\n"
    "    assert og[tuple(v.T)].tolist() == ([1, 1, 1, 1] if up else [1, 0, 0, 0]), (kind, v.tolist())\n"
    "    joined += up\n"
    "assert joined == 4, joined\n"
    # an element the union-find cannot take (no x neighbours): the frontier engine, announced by its trace lines
    "s = np.zeros((3, 3, 3), np.uint8); s[:, 1, 1] = 1\n"
    "p = R.noise(6)\n"
    "sys.stderr.write('zonly-begin\\n'); sys.stderr.flush()\n"
    "og = flood(p.astype(np.int16) * 100, R.flood_seeds(p, 6), s, R.flood_barriers(p.shape, 4))\n"
    "sys.stderr.write('zonly-end\\n'); sys.stderr.flush()\n"
    "assert np.array_equal(og, R.flood_by_label(p, R.flood_seeds(p, 6), 1, s, R.flood_barriers(p.shape, 4)))\n"
    "print('ccl-ok')\n")


def test_union_find_engine_from_the_start_in_a_fresh_process(ivxlib, oracle):
    """IVX_FLOOD_MODE=ccl (read once per process): floods of the cases A..E under 6 / 18 / 26 with seeds in several
    components (also ones that lie across an x tile boundary), on an out-of-range voxel and in the two far corners,
    barriers pre-filled; a point-symmetric element that is none of the three (the x-increasing stairs join, the
    x-decreasing ones and the two-axis ones do not); an element without x neighbours, which must take the frontier.
    IVX_FLOOD_TRACE makes the frontier announce each round: such lines appear for the last element only."""
    env = dict(os.environ, IVX_FLOOD_MODE="ccl", IVX_FLOOD_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _CCL_CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ccl-ok" in r.stdout, r.stdout + r.stderr
    head, _, rest = r.stderr.partition("zonly-begin")
    inside, _, tail = rest.partition("zonly-end")
    assert "ivx flood: round" in inside and "ivx flood: round" not in head + tail, r.stderr[-2000:]


def test_region_grow_on_the_corridor_is_completed_by_the_union_find(ivxlib, oracle):
    """DeviceVolume.region_grow on the corridor, twice per structure: the host escapes to the union-find engine once it has
    seen round 48 start and adds one to the round count (CCL_ESCAPE_ROUNDS in flood_run_impl), and `mask[reached] = 254`
    is queued behind the completed flood: same mask, same out_mask as the oracle.  Whether the 26-neighbour flood needs 48
    rounds here as well is not asserted: the escape has to show once over the loop."""
    from invesalius3_amd.device import DeviceVolume
    img = R.serpentine()
    vol = DeviceVolume(img, spacing=(1.0, 1.0, 1.0))
    seen = []
    try:
        for conn in (1, 3):
            s = generate_binary_structure(3, conn).astype(np.uint8)
            for _ in range(2):
                vol.zero_out_mask()
                vol.threshold(1, 1)
                rounds = vol.region_grow([(0, 0, 1)], 1, 1, s, fill=1, select_value=254)
                assert rounds >= 1, rounds
                seen.append(rounds)
            mask = np.where(img == 1, 255, 0).astype(np.uint8)
            out = np.zeros(img.shape, np.uint8)
            oracle.floodfill_threshold(img, [(0, 0, 1)], 1, 1, 1, s, out)
            mask[out.astype(bool)] = 254
            assert np.array_equal(vol.download_out_mask(), out), conn
            assert np.array_equal(vol.download_mask(), mask), conn
            assert (mask == 254).sum() > 30 * 1100 and (mask[2] == 255).any() == (conn == 1), conn
    finally:
        vol.close()
    assert max(seen) >= 49, seen
