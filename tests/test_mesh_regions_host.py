"""CPU: the restatement of the surface connectivity rules (tests/_mesh_regions_ref.py) against a mesh numbered by hand,
the seed range check that runs before any GPU call, and the headless driver's --largest / --surface-seed exclusivity."""
import numpy as np
import pytest

import _mesh_regions_ref as R


def test_restatement_on_the_hand_numbered_mesh():
    v, f = R.hand_mesh()
    tl, vl, n = R.region_labels(len(v), f)
    assert n == 4
    assert np.array_equal(tl, R.HAND_TRI_LABELS) and np.array_equal(vl, R.HAND_VERT_LABELS)
    parts, table = R.split(v, f)
    assert np.array_equal(table, R.HAND_TABLE)
    # part 0: two triangles that share one point; part 1 keeps the triangle with the repeated index
    assert np.array_equal(parts[0][1], [[0, 1, 2], [2, 3, 4]]) and np.array_equal(parts[0][0], v[:5])
    assert np.array_equal(parts[1][1], [[0, 1, 2], [1, 2, 3], [2, 3, 3]]) and np.array_equal(parts[1][0], v[5:9])
    assert np.array_equal(parts[2][0], v[10:15]) and np.array_equal(parts[3][0], v[15:19])
    for pv, pf in parts:
        assert pf.dtype == np.int32 and pv.dtype == np.float32
    # every triangle is in exactly one part, as the same three points
    soup = np.concatenate([pv[pf] for pv, pf in parts])
    assert np.array_equal(soup, v[f][np.argsort(tl, kind="stable")])
    # largest: regions 1 and 2 tie with three triangles, the lower number wins
    lv, lf = R.largest(v, f)
    assert np.array_equal(lv, parts[1][0]) and np.array_equal(lf, parts[1][1])


def test_restatement_seeds_and_nearest():
    v, f = R.hand_mesh()
    parts, _ = R.split(v, f)
    sv, sf = R.seeded(v, f, [16, 0, 16])  # regions 3 and 0, a duplicate
    assert np.array_equal(sv, np.concatenate([v[:5], v[15:19]]))
    assert np.array_equal(sv[sf], v[f][[0, 5, 6, 9]])
    sv, sf = R.seeded(v, f, [9])          # the unused point
    assert sv.shape == (0, 3) and sf.shape == (0, 3)
    sv, sf = R.seeded(v, f, [])
    assert sv.shape == (0, 3) and sf.shape == (0, 3)
    w = np.concatenate([v, v[3:4]])       # a duplicated point: the smaller id wins
    assert R.nearest_point(w, w[19].astype(np.float64)) == 3
    assert R.nearest_point(np.zeros((0, 3), np.float32), (0, 0, 0)) == -1


def test_restatement_shuffled_disjoint_triangles_is_fast_and_ordered():
    n = 5000
    rng = np.random.default_rng(1)
    f = rng.permutation(3 * n).astype(np.int32).reshape(n, 3)
    tl, vl, nr = R.region_labels(3 * n, f)
    assert nr == n and np.array_equal(tl, np.arange(n)) and np.array_equal(vl[f[:, 1]], np.arange(n))


@pytest.mark.parametrize("bad", [[-1], [0, 19], [3, 1 << 40]])
def test_seed_range_is_checked_before_any_gpu_call(bad, monkeypatch):
    from invesalius3_amd import _lib as L
    from invesalius3_amd import polydata_utils as pu
    monkeypatch.setattr(L, "lib", lambda: pytest.fail("the library was reached"))
    v, f = R.hand_mesh()
    with pytest.raises(ValueError, match="outside"):
        pu.JoinSeedsParts(v, f, bad)
    with pytest.raises(ValueError, match="outside"):
        pu.DeviceMesh(None, len(v), None, len(f)).select_seeded(bad)
    with pytest.raises(ValueError):
        pu.JoinSeedsParts(v, f, [0.5])


def test_headless_largest_and_surface_seed_exclude_each_other(capsys):
    from invesalius3_amd import headless
    with pytest.raises(SystemExit) as e:
        headless.main(["x.inv3", "--threshold", "1", "2", "--largest", "--surface-seed", "1", "2", "3"])
    assert e.value.code == 2 and "not allowed with" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        headless.main(["x.inv3", "--threshold", "1", "2", "--surface-seed", "1", "2"])
    assert e.value.code == 2 and "triples" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        headless.main(["x.inv3", "--split-min-triangles", "5"])
    assert e.value.code == 2
