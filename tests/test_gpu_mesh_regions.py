"""Surface connectivity tools on the GPU (csrc/k_meshparts.hip): region labels, the split into parts, seeded parts,
per-part mass and the nearest point, array for array against the numpy restatement of the rules (tests/_mesh_regions_ref.py).
The radix partition has 8-bit digits: its pass-count edges are 256 and 65 536 keys (triangles: R keys, points: R + 1)."""
import ctypes

import numpy as np
import pytest

import _mesh_regions_ref as R
from conftest import synth_volume

pytestmark = pytest.mark.gpu


def _strips(sizes, seed, spare=3):
    """disjoint triangle strips of the given sizes, face order shuffled, point ids permuted, `spare` unused points"""
    rng = np.random.default_rng(seed)
    faces, base = [], 0
    for n in sizes:
        i = np.arange(n, dtype=np.int64) + base
        faces.append(np.stack([i, i + 1, i + 2], axis=1))
        base += n + 2
    f = np.concatenate(faces)
    nv = base + spare
    perm = rng.permutation(nv)
    f = perm[f][rng.permutation(len(f))]
    return rng.standard_normal((nv, 3)).astype(np.float32), f.astype(np.int32)


def _check_split(v, f, by_part=True):
    from invesalius3_amd import polydata_utils as pu
    from invesalius3_amd import surface_process as sp
    tl0, vl0, n0 = R.region_labels(len(v), f)
    tl, n = sp.region_labels(v, f)
    assert n == n0 and np.array_equal(tl, tl0)
    assert np.array_equal(sp.vertex_region_labels(v, f), vl0)
    gv0, gf0, tb0 = R.split_grouped(v, f)
    gv, gf, tb = pu.split_arrays(v, f)
    assert np.array_equal(tb, tb0) and np.array_equal(gf, gf0) and np.array_equal(gv, gv0)
    if by_part:
        parts0, table0 = R.split(v, f)
        assert np.array_equal(table0, tb0)
        parts = pu.SplitDisconectedParts(v, f)
        assert len(parts) == len(parts0)
        for (pv, pf), (pv0, pf0) in zip(parts, parts0):
            assert np.array_equal(pf, pf0) and np.array_equal(pv, pv0)
    return gv, gf, tb


def test_hand_mesh_and_empty_mesh(ivxlib):
    from invesalius3_amd import polydata_utils as pu
    from invesalius3_amd import surface_process as sp
    v, f = R.hand_mesh()
    tl, n = sp.region_labels(v, f)
    assert n == 4 and np.array_equal(tl, R.HAND_TRI_LABELS)
    assert np.array_equal(sp.vertex_region_labels(v, f), R.HAND_VERT_LABELS)
    _, _, tb = _check_split(v, f)
    assert np.array_equal(tb, R.HAND_TABLE)
    lv, lf = pu.SelectLargestPart(v, f)
    lv0, lf0 = R.largest(v, f)
    assert np.array_equal(lv, lv0) and np.array_equal(lf, lf0)
    # nothing in, nothing out
    v0, f0 = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    tl, n = sp.region_labels(v0, f0)
    assert n == 0 and tl.shape == (0,)
    assert pu.SplitDisconectedParts(v0, f0) == []
    assert np.array_equal(sp.vertex_region_labels(v[:4], f0), [-1] * 4) and pu.SplitDisconectedParts(v[:4], f0) == []
    sv, sf = pu.JoinSeedsParts(v0, f0, [])
    assert sv.shape == (0, 3) and sf.shape == (0, 3)
    with pytest.raises((ValueError, IndexError)):
        sp.region_labels(v, np.array([[0, 1, 19]], np.int32))


def test_interleaved_strips_cross_every_block_size(ivxlib):
    sizes = [1] + [s for k in range(6, 14) for s in (2 ** k - 1, 2 ** k, 2 ** k + 1)]
    v, f = _strips(sizes, seed=11)
    _, _, tb = _check_split(v, f)
    assert sorted(tb[:, 1].tolist()) == sorted(sizes)


@pytest.mark.parametrize("nreg", [255, 256, 257, 65535, 65536, 65537])
def test_region_counts_at_the_radix_pass_edges(ivxlib, nreg):
    v, f = _strips([1] * (nreg - 1) + [3000], seed=nreg)
    _, _, tb = _check_split(v, f, by_part=False)
    assert len(tb) == nreg and tb[:, 1].max() == 3000


@pytest.mark.parametrize("nkeys", [1, 2, 256, 257, 65536, 65537])
def test_partition_is_the_stable_argsort(ivxlib, nkeys):
    from invesalius3_amd import _lib as L
    from invesalius3_amd.device import DeviceBuffer
    rng = np.random.default_rng(nkeys)
    n = 20001
    keys = rng.integers(0, nkeys, n).astype(np.uint32)
    keys[rng.random(n) < 0.8] = nkeys // 2  # most items in ONE key, as on a real surface
    dk, do, df = DeviceBuffer(n * 4), DeviceBuffer(n * 4), DeviceBuffer((nkeys + 1) * 4)
    dk.upload(keys)
    L.check(L.lib().ivx_dev_partition_u32(dk.ptr, ctypes.c_int64(n), ctypes.c_uint32(nkeys), do.ptr, df.ptr, None))
    L.synchronize()
    assert np.array_equal(do.download((n,), np.uint32), np.argsort(keys, kind="stable"))
    assert np.array_equal(df.download((nkeys + 1,), np.uint32), np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=nkeys))]))
    for b in (dk, do, df):
        b.close()


@pytest.fixture(scope="module")
def noisy(ivxlib):
    """a marching-cubes surface with specks: one dominant region and hundreds of small ones"""
    from invesalius3_amd import surface_process as sp
    img = synth_volume((40, 48, 80), seed=9)
    img[np.random.default_rng(3).random(img.shape) < 0.003] = 2500
    v, f = sp.marching_cubes_indexed(img, (0.5, 0.5, 1.0), [300.0], 0, True, True, True, float(np.iinfo(np.int16).min), 1)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def test_marching_cubes_mesh_and_largest_part(ivxlib, noisy):
    from invesalius3_amd import surface_process as sp
    v, f = noisy
    gv, gf, tb = _check_split(v, f, by_part=False)
    assert len(tb) > 100 and tb[:, 1].max() > 0.5 * len(f)
    big = int(np.argmax(tb[:, 1]))
    to, tn, vo, vn = tb[big]
    kv, kf, nreg = sp.keep_largest(v, f)
    assert nreg == len(tb)
    assert np.array_equal(gf[to:to + tn], kf) and np.array_equal(gv[vo:vo + vn], kv)


def test_seeded_parts(ivxlib, noisy):
    from invesalius3_amd import polydata_utils as pu
    v, f = R.hand_mesh()
    for ids in ([16, 0, 16], [5], [9], [9, 12], [], np.array([18, 14], np.int64)):
        sv, sf = pu.JoinSeedsParts(v, f, ids)
        sv0, sf0 = R.seeded(v, f, ids)
        assert np.array_equal(sf, sf0) and np.array_equal(sv, sv0), ids
    assert len(pu.JoinSeedsParts(v, f, [16, 0, 16])[1]) == 4 and len(pu.JoinSeedsParts(v, f, [9])[1]) == 0
    v, f = noisy
    ids = [int(f[0, 0]), int(f[-1, 2]), int(f[len(f) // 2, 1]), int(f[0, 0])]
    sv, sf = pu.JoinSeedsParts(v, f, ids)
    sv0, sf0 = R.seeded(v, f, ids)
    assert len(sf0) and np.array_equal(sf, sf0) and np.array_equal(sv, sv0)


def _balls_mesh():
    """balls of 8 to a few thousand triangles: parts on both sides of 64 and of 1024 triangles"""
    from invesalius3_amd import surface_process as sp
    z, y, x = np.mgrid[:30, :30, :150]
    m = np.zeros(z.shape, np.uint8)
    cx = 4
    for r in (0, 1, 0, 2, 3, 0, 4, 6, 9, 12, 1, 0):
        cx += r + 2
        m[(z - 14) ** 2 + (y - 15) ** 2 + (x - cx) ** 2 <= r * r] = 255
        cx += r + 2
    assert cx < 148
    return sp.marching_cubes_indexed(m, (0.5, 0.75, 1.25), [127.0])


def test_per_part_mass_and_run_to_run_identity(ivxlib):
    from invesalius3_amd import polydata_utils as pu
    from invesalius3_amd import surface_process as sp
    v, f = _balls_mesh()
    mesh = pu.DeviceMesh.upload(v, f)
    parts = mesh.split()
    tb = parts.table
    full = parts.mass_properties_full()
    gv, gf = parts.verts.download((parts.nverts, 3), np.float32), parts.faces.download((parts.ntris, 3), np.int32)
    # the wave-per-part kernel and the two-kernel path share the terms, not the order of the sums: both limits on both sides
    variants = {0: full, 64: parts.mass_properties_full(64), 1 << 30: parts.mass_properties_full(1 << 30)}
    assert tb[:, 1].max() > 1024 and np.count_nonzero(tb[:, 1] > 64) > 1 and np.count_nonzero(tb[:, 1] <= 64) > 1
    for r, (to, tn, vo, vn) in enumerate(tb.tolist()):
        want = sp.mass_properties_full(gv[vo:vo + vn], gf[to:to + tn])
        for small_max, got in variants.items():
            # double sums in a different order: 1e-10 relative (tests/test_gpu_mesh.py); the integer weights are exact
            assert got[r, 0] == pytest.approx(want[0], rel=1e-10) and got[r, 1] == pytest.approx(want[1], rel=1e-10), (r, small_max)
            for q in (2, 3, 4):
                assert got[r, q] == pytest.approx(want[q], rel=1e-10, abs=1e-9), (r, small_max)
            assert np.array_equal(got[r, 5:], want[5:]), (r, small_max)
    assert np.array_equal(parts.mass_properties(), full[:, :2])
    assert np.array_equal(pu.parts_mass_properties(gv, gf, tb), full[:, :2])
    # a second run: the same bytes everywhere
    again = mesh.split()
    assert np.array_equal(again.table, tb) and np.array_equal(again.mass_properties_full(), full)
    assert np.array_equal(again.verts.download((parts.nverts, 3), np.float32), gv)
    assert np.array_equal(again.faces.download((parts.ntris, 3), np.int32), gf)
    l1, n1 = mesh.region_labels()
    l2, n2 = mesh.region_labels()
    assert n1 == n2 == parts.n and np.array_equal(l1, l2)
    for m in (again, parts, mesh):
        m.close()


def test_device_resident_path_gives_the_host_path_bytes(ivxlib, noisy):
    from invesalius3_amd import polydata_utils as pu
    from invesalius3_amd import surface_process as sp
    v, f = noisy
    mesh = pu.DeviceMesh.upload(v, f)
    tl, n = mesh.region_labels()
    tl0, n0 = sp.region_labels(v, f)
    assert n == n0 and np.array_equal(tl, tl0)
    parts = pu.SplitDisconectedParts(mesh)
    gv, gf, tb = pu.split_arrays(v, f)
    assert parts.n == n and np.array_equal(parts.table, tb)
    assert np.array_equal(parts.verts.download((parts.nverts, 3), np.float32), gv)
    assert np.array_equal(parts.faces.download((parts.ntris, 3), np.int32), gf)
    order = np.argsort(-tb[:, 1], kind="stable")
    for r in [int(order[0]), int(order[1]), int(order[-1]), 1]:
        to, tn, vo, vn = tb[r]
        view = parts.part(r)  # (odd offsets: a view is 4-byte aligned only)
        pv, pf = view.download()
        assert np.array_equal(pv, gv[vo:vo + vn]) and np.array_equal(pf, gf[to:to + tn])
        assert pu.bounds(view) == pu.bounds(pv)
        assert np.array_equal(parts.download(r)[1], pf)
        # the kernels a view can reach: keep largest and the seeded select of a single part give the part back
        for same in (view.keep_largest(), view.select_seeded([0])):
            sv, sf = same.download()
            assert np.array_equal(sv, pv) and np.array_equal(sf, pf)
            same.close()
    big = pu.SelectLargestPart(mesh)
    kv, kf, _ = sp.keep_largest(v, f)
    bv, bf = big.download()
    assert np.array_equal(bv, kv) and np.array_equal(bf, kf)
    ids = [int(f[0, 0]), int(f[-1, 2])]
    sel = pu.JoinSeedsParts(mesh, point_id_list=ids)
    sv0, sf0 = pu.JoinSeedsParts(v, f, ids)
    sv, sf = sel.download()
    assert np.array_equal(sv, sv0) and np.array_equal(sf, sf0)
    for m in (sel, big, parts, mesh):
        m.close()


def test_nearest_point(ivxlib, noisy):
    from invesalius3_amd import polydata_utils as pu
    v, _ = noisy
    rng = np.random.default_rng(2)
    w = np.concatenate([v, v[100:103], v[:1]])  # duplicated points: the smaller id wins
    mesh = pu.DeviceMesh.upload(w, np.zeros((0, 3), np.int32))
    queries = [w[len(v)].astype(np.float64), w[-1].astype(np.float64), w[len(v) + 2].astype(np.float64) + 1e-9]
    queries += [rng.uniform(w.min(0), w.max(0)) for _ in range(5)] + [np.array([1e6, -1e6, 3.0])]
    for q in queries:
        want = R.nearest_point(w, q)
        assert pu.nearest_point(w, q) == want and mesh.nearest_point(q) == want
    assert pu.nearest_point(w, queries[0]) == 100 and pu.nearest_point(w, queries[1]) == 0
    assert pu.nearest_point(np.zeros((0, 3), np.float32), (0, 0, 0)) == -1
    assert pu.nearest_point(w[:1], (5, 5, 5)) == 0
    mesh.close()
