"""The inputs of tests/test_gpu_ccl.py, checked where no GPU is needed: the cases must really have what they are there
for (components across every tile boundary, components of exactly `size` and `size + 1` voxels, the component counts
they were built to have), and the numpy / scipy recipe of tests/_ccl_ref.py must agree with the oracle on every input
the GPU tests use, so that those compare the kernels with two references that were written apart and say the same."""
import numpy as np
import pytest
from scipy import ndimage

import _ccl_ref as R

CONNS = (6, 18, 26)
BUILT = ("checker", "solid", "stairs", "edges")


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("case", R.CASES)
def test_recipe_and_oracle_agree_3d(oracle, case, conn):
    m = R.mask_of(R.pattern(case, conn))
    changed = []
    for size in R.fill_sizes(case, conn):
        want, ret = R.fill_holes(m, "3D", conn, "AXIAL", 0, size)
        orc = m.copy()
        ret0 = oracle.mask_fill_holes_auto(orc, "3D", conn, "AXIAL", 0, size)
        assert ret == ret0 and np.array_equal(want, orc), size
        assert not want[0].any() and not want[:, 0].any() and not want[:, :, 0].any()
        changed.append(ret)
    assert any(changed)


@pytest.mark.parametrize("orientation", ["AXIAL", "CORONAL", "SAGITAL"])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("case", ["noise", "stairs"])
def test_recipe_and_oracle_agree_2d(oracle, case, conn, orientation):
    m = R.mask_of(R.pattern_2d(case, conn))
    changed = 0
    for index in R.indices_2d(case, orientation):
        for size in R.sizes_2d(case):
            want, ret = R.fill_holes(m, "2D", conn, orientation, index, size)
            orc = m.copy()
            ret0 = oracle.mask_fill_holes_auto(orc, "2D", conn, orientation, index, size)
            assert ret == ret0 and np.array_equal(want, orc), (index, size)
            changed += ret
    assert changed


@pytest.mark.parametrize("conn", CONNS)
def test_noise_reaches_every_boundary_and_both_sides_of_the_size_rule(conn):
    labels, counts = R.labelled("noise", conn)
    for axis, lo in ((2, 511), (2, 1023), (1, 7), (0, 3)):
        assert len(R.straddling(labels, axis, lo)) >= 3, (axis, lo)
    assert (counts[1:] == R.SIZE_A).sum() >= 1 and (counts[1:] == R.SIZE_A + 1).sum() >= 1
    sizes = R.fill_sizes("noise", conn)
    assert sizes[:3] == [1, 5, 6] and sizes[3] == counts[1:].max() + 1 < counts[0]  # label 0 stays the one large label
    # a small component inside the partial last word, whose padding bits must not be counted
    tail = np.unique(labels[:, :, 1024:])
    assert ((counts[tail[tail > 0]] <= R.SIZE_A).sum()) >= 1
    assert -(-R.SHAPES["noise"][2] // 64) * R.SHAPES["noise"][0] * R.SHAPES["noise"][1] > 4096  # two scan blocks


def test_component_counts_of_the_built_cases():
    def comps(case, conn):
        counts = R.labelled(case, conn)[1]
        return len(counts) - 1, sorted(set(counts[1:].tolist())), int(counts[0])

    assert comps("checker", 6) == (23175, [1], 23175)
    assert comps("checker", 18) == comps("checker", 26) == (1, [23175], 23175)
    for conn in CONNS:
        assert comps("solid", conn) == (2, [18540], 9270)
    chains = R.stairs_chains()
    n3, n2 = sum(k == "zyx" for k, _ in chains), sum(k != "zyx" for k, _ in chains)
    assert (n3, n2) == (9, 12) and all(len(v) == R.CHAIN for _, v in chains)
    assert comps("stairs", 26)[:2] == (n3 + n2, [R.CHAIN])
    assert comps("stairs", 18)[:2] == (n2 + n3 * R.CHAIN, [1, R.CHAIN])
    assert comps("stairs", 6)[:2] == ((n3 + n2) * R.CHAIN, [1])
    bars = sorted(len(v) for _, v in R.edge_bars())
    assert bars == [1, 5, 5, 5, 6, 6, 7, 599, 600]
    for conn in CONNS:
        counts = R.labelled("edges", conn)[1]
        assert sorted(counts[1:].tolist()) == bars


def test_stairs_cross_the_boundaries_they_name():
    """per x boundary: a three-axis chain whose one step crosses x, y = 7|8 and z = 3|4 together, three-axis chains in
    both x directions inside one y/z tile, two-axis chains in both x directions across y = 7|8 and across z = 3|4"""
    for b in (192, 512, 1024):
        seen = set()
        for kind, v in R.stairs_chains():
            if not (v[:, 2].min() < b <= v[:, 2].max()):
                continue
            step = np.flatnonzero((v[:-1, 2] < b) != (v[1:, 2] < b))
            assert len(step) == 1 and (np.abs(np.diff(v, axis=0)).max(0) <= 1).all()
            a, c = v[step[0]], v[step[0] + 1]
            up = bool(c[2] > a[2])
            ycross, zcross = {a[1], c[1]} == {7, 8}, {a[0], c[0]} == {3, 4}
            one_tile = len(set(v[:, 0] // 4)) == 1 and len(set(v[:, 1] // 8)) == 1
            seen.add((kind, up, bool(ycross), bool(zcross), one_tile))
        assert {("zyx", True, False, False, True), ("zyx", False, False, False, True), ("yx", True, True, False, False),
                ("yx", False, True, False, False), ("zx", True, False, True, False), ("zx", False, False, True, False)} <= seen
        assert ("zyx", b == 512, True, True, False) in seen


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("case", BUILT)
def test_recipe_agrees_with_the_components_as_built(case, conn):
    p = R.pattern(case, conn)
    m = R.mask_of(p)
    groups = R.known_groups(case, conn)
    assert sum(int(w.sum()) for _, w in groups) == int(p.sum())
    for size in R.fill_sizes(case, conn):
        want, ret = R.fill_holes(m, "3D", conn, "AXIAL", 0, size)
        inner, ret1 = R.fill_holes_known(p, groups, size)
        assert ret == ret1 and np.array_equal(want[1:, 1:, 1:], inner), size


def test_what_the_edge_sizes_do():
    """the statements of the cases, spelled out once on the recipe"""
    inner = lambda case, conn, size: R.fill_holes(R.mask_of(R.pattern(case, conn)), "3D", conn, "AXIAL", 0, size)
    p = R.checker()
    out, ret = inner("checker", 6, 1)
    assert ret and (out[1:, 1:, 1:][p] == 254).all() and (out[1:, 1:, 1:][~p] == 255).all()
    for conn in (18, 26):
        out, ret = inner("checker", conn, 23174)
        assert not ret and np.array_equal(out, R.mask_of(p))
    for conn in CONNS:
        out, ret = inner("checker", conn, 23175)
        assert ret and (out[1:, 1:, 1:] == 254).all()  # label 0 has exactly `size` voxels: the voxels > 127 go too
        out, ret = inner("solid", conn, 18539)
        assert ret and (out[3] == 254)[1:, 1:].all() and not (out[1:, 1:, 1:][R.solid()] == 254).any()  # the plane alone
        out, ret = inner("solid", conn, 9269)
        assert not ret
        out, ret = inner("solid", conn, 18540)
        assert ret and (out[1:, 1:, 1:] == 254).all()
    bars = dict(R.edge_bars())
    for size, flipped in ((5, {"origin5", "tile5", "tail5"}), (6, {"last_word", "word6"}), (7, {"ell7"}),
                          (599, {"bar599"}), (600, {"bar600"})):
        out, ret = inner("edges", 26, size)
        for name, v in bars.items():
            assert (out[1:, 1:, 1:][tuple(v.T)] == 254).all() == (len(v) <= size), (size, name)
        assert {n for n, v in bars.items() if len(v) == size} == flipped  # what this size adds to the size before


@pytest.mark.parametrize("conn", [1, 2, 3])
def test_flood_statement_with_scipy_label_agrees_with_the_oracle(oracle, conn):
    c3 = {1: 6, 2: 18, 3: 26}[conn]
    p = R.noise(c3)
    img = p.astype(np.int16) * 100
    seeds = R.flood_seeds(p, c3)
    labels = R.labelled("noise", c3)[0]
    hit = {int(labels[z, y, x]) for x, y, z in seeds}
    assert 0 in hit and len(hit) >= 5  # a seed outside the range, seeds in several components
    assert any(lab in hit for lab in R.straddling(labels, 2, 511)) and any(lab in hit for lab in R.straddling(labels, 2, 1023))
    strct = ndimage.generate_binary_structure(3, conn)
    out0 = R.flood_barriers(p.shape, conn)
    want = R.flood_by_label(p, seeds, 1, strct, out0)
    orc = out0.copy()
    oracle.floodfill_threshold(img, seeds, 50, 150, 1, strct, orc)
    assert np.array_equal(want, orc) and (want != out0).sum() > 20


def test_serpentine_is_one_corridor_across_both_tile_boundaries():
    img = R.serpentine()
    labels, n = ndimage.label(img[1] == 1, ndimage.generate_binary_structure(2, 1))
    assert n == 1 and img.shape == (3, 60, 1100) and (img[1] == 1).sum() == 30 * 1100 + 30
    assert not img[0].any() and img[2].any()
    # 30 rows of 18 flood tiles (64 voxels) each, joined at alternating ends: the frontier needs a round per tile hop
    assert 30 * -(-1100 // 64) > 10 * 48
