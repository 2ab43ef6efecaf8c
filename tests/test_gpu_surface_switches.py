"""GPU: the surface tail's kernels -- context-aware smoothing (csrc/k_smooth.hip), hole filling and point normals (k_meshtail.hip), the
geodesic graph builder (k_meshgeo.hip), keep-largest and mass properties (k_mesh.hip, mesh_regions.h, scan_u32.h) -- on either
side of every switch between two code paths, on the meshes of _surface_switch_cases.py.  Marching-cubes meshes, which the other
GPU tests of these files run on, keep to valence 6 .. 12 and short rims and cross none of these switches.  Every comparison is
np.array_equal on values or on their bits, against the reference each kernel family already has; the one exception, the mass
sums, states its bound.  tests/test_surface_switch_cases_host.py checks that every case stands where it is said to."""
import ctypes
import math

import numpy as np
import pytest

import _geodesic_ref as G
import _mesh_tail_ref as ref
import _surface_switch_cases as S

pytestmark = pytest.mark.gpu

OPTS = (0.7, 3.0, 0.5, 10)  # task_navigator.py:827 defaults: angle, max distance, min weight, steps


# ---- smoothing -------------------------------------------------------------------------------------------------------------
def _smooth_both_ways(oracle, v, f, hub):
    """the mesh through rs.Mesh.from_indexed + rs.ca_smoothing and through ivx_context_aware_smoothing with flags and weights out:
    vertices, staircase flags and weights are the oracle's"""
    from invesalius3_amd import _lib as L
    from invesalius3_amd import invesalius_rs as rs
    nrm = oracle.mesh_face_normals(v, f)
    want = v.copy()
    flags0, w0 = oracle.context_aware_smoothing(want, S.faces4(f), nrm, *OPTS, details=True)
    assert not np.array_equal(want[hub], v[hub])
    mesh = rs.Mesh.from_indexed(v.copy(), f)
    assert np.array_equal(mesh.normals, nrm)
    rs.ca_smoothing(mesh, *OPTS)
    assert mesh.vertices.dtype == v.dtype and np.array_equal(mesh.vertices, want), int((mesh.vertices != want).any(axis=1).sum())
    got = v.copy()
    flags, w = np.zeros(len(v), np.uint8), np.zeros(len(v), np.float64)
    L.check(L.lib().ivx_context_aware_smoothing(L.ptr(got), L.F64 if v.dtype == np.float64 else L.F32, ctypes.c_int64(len(got)),
                                                L.ptr(f), ctypes.c_int64(len(f)), L.ptr(nrm), ctypes.c_double(OPTS[0]),
                                                ctypes.c_double(OPTS[1]), ctypes.c_double(OPTS[2]), ctypes.c_int(OPTS[3]),
                                                L.ptr(flags), L.ptr(w)))
    assert np.array_equal(flags, flags0) and np.array_equal(w, w0) and np.array_equal(got, want)


@pytest.mark.parametrize("vdtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,k", S.FAN_LADDER)
def test_fan_ladder_across_the_register_limit(ivxlib, oracle, name, k, vdtype):
    """11 / 12 / 13 incident faces at the hub (register sort | in-place sort) and 12 | 13 .. 26 neighbours from at most 12 faces
    (all in registers | the tail spilled to global memory), the hub as vertex 0, as vertex 3 (Q-M1) and as the last one.  The
    float64 runs are the ones that show the neighbour order (test_float64_fans_show_the_neighbour_order)."""
    for hub_id in S.HUB_IDS:
        v, f, hub = S.FANS[name](k, hub_id, dtype=vdtype)
        _smooth_both_ways(oracle, v, f, hub)


@pytest.mark.parametrize("kind", ["degenerate", "duplicate"])
@pytest.mark.parametrize("name,k", S.FAN_LADDER)
def test_fan_ladder_with_a_repeated_face(ivxlib, oracle, name, k, kind):
    """one face listed twice at the hub ([hub, hub, a]: walked once) or one triangle twice in the face list (two ids: walked twice,
    nothing new the second time).  What these cases pin is the adjacency order, for the hub as vertex 3 too: the staircase flags
    are all ones by quirk Q-M2 (the first face of any vertex already reports it), so the Q-M1 loop of k_sm_staircase ends at its
    first face and its branch for a repeated face is reached by no input."""
    for vdtype in (np.float64, np.float32):
        for hub_id in S.HUB_IDS:
            v, f, hub = S.with_repeat(*S.FANS[name](k, hub_id, dtype=vdtype), kind)
            _smooth_both_ways(oracle, v, f, hub)


@pytest.mark.parametrize("vdtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("side", ["far", "near"])
def test_propagate_tie_goes_to_the_smaller_seed_id(ivxlib, oracle, side, vdtype):
    from invesalius3_amd import invesalius_rs as rs
    v, f, seeds, info = S.tie_strip(side)
    v = v.astype(vdtype)
    w = rs.propagate_weights(v, f, seeds, 10.0, 0.5)
    assert np.array_equal(w, oracle.mesh_propagate_weights(v, f, seeds, 10.0, 0.5))
    small = min(info["seeds"])
    for d in info["dangling"]:  # (what the host test derives, once more on the kernel's own numbers)
        assert w[d] == S.weight_of(float(((v[d].astype(np.float64) - v[small]) ** 2).sum()), 10.0, 0.5)


@pytest.mark.parametrize("vdtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_propagate_distance_equal_to_tmax_is_inside(ivxlib, oracle, vdtype):
    from invesalius3_amd import invesalius_rs as rs
    v, f, seeds, ids = S.edge_345()
    v = v.astype(vdtype)
    w = rs.propagate_weights(v, f, seeds, 5.0, 0.5)
    assert np.array_equal(w, oracle.mesh_propagate_weights(v, f, seeds, 5.0, 0.5))
    assert w[ids["C"]] > 0.5 and w[ids["E"]] > 0.5 and w[ids["P"]] == 0.5  # P is in (weight 1 - 5 / 5 -> bmin) and passes the seed on
    below = float(np.nextafter(5.0, 0.0))
    w = rs.propagate_weights(v, f, seeds, below, 0.5)
    assert np.array_equal(w, oracle.mesh_propagate_weights(v, f, seeds, below, 0.5)) and w.tolist() == [1.0, 0.5, 0.5, 0.5, 0.5]


def test_propagate_over_hundreds_of_rounds(ivxlib, oracle):
    from invesalius3_amd import invesalius_rs as rs
    v, f = G.strip(300)
    for end in (0, len(v) - 1):
        seeds = np.zeros(len(v), np.uint8)
        seeds[end] = 1
        w = rs.propagate_weights(v, f, seeds, 1e9, 0.5)
        assert np.array_equal(w, oracle.mesh_propagate_weights(v, f, seeds, 1e9, 0.5))
        assert (w > 0.5).all() and w[end] == 1.0


# ---- hole filling and point normals ------------------------------------------------------------------------------------------
def _tail_equals_the_rules(v, f, hole, combos=((True, 80.0), (True, 30.0), (False, 80.0), (False, 30.0))):
    """fill_holes, then point_normals of the filled mesh, array for array against tests/_mesh_tail_ref.py.  KNOWN LIMIT: the order of
    the corners inside one fan only enters a float64 sum that is then cast to float32, so what is pinned here is which fan a
    corner is in and which point id the fan gets -- not that inner order."""
    from invesalius3_amd import surface_process as sp
    gv, gf, gn = sp.fill_holes(v, f, hole)
    rv, rf, rn = ref.fill_holes(v, f, hole)
    assert gn == rn and np.array_equal(gf, rf) and np.array_equal(gv.view(np.uint32), rv.view(np.uint32))
    extra = {}
    for splitting, angle in combos:
        g = sp.point_normals(gv, gf, angle, splitting, True)
        r = ref.point_normals(rv, rf, angle, splitting, True)
        assert np.array_equal(g[1], r[1]), (splitting, angle, "faces")
        for k in (0, 2, 3):
            assert g[k].shape == r[k].shape and np.array_equal(g[k].view(np.uint32), r[k].view(np.uint32)), (splitting, angle, k)
        extra[(splitting, angle)] = len(r[0]) - len(rv)
    return rv, rf, rn, extra


@pytest.mark.parametrize("k", [3, 63, 64, 65])
def test_open_fan_at_the_rim_turns_through_64_faces(ivxlib, k):
    """the hub lies on the rim with k faces between its two rim edges: up to 64 the rim closes (k + 2 cap triangles), with 65 the
    chain is given up and the whole rim stays open -- defined behaviour on both sides.  From 63 on the hub's corners also go
    through the workgroup sort."""
    v, f, hub = S.open_fan(k, 0, dtype=np.float32)
    rv, rf, holes, _ = _tail_equals_the_rules(v, f, 300.0)
    if k <= S.RIM_TURNS:
        assert holes == 1 and len(rf) == len(f) + k + 2
    else:
        assert holes == 0 and np.array_equal(rf, f)


@pytest.mark.parametrize("m", [47, 48, 49, 64, 65, 255, 256, 257, 300])
def test_cone_cap_across_the_lane_sort_limit(ivxlib, m):
    """apex and cap centroid have m corners: one lane's insertion sort up to 48, the workgroup's bitonic network from 49, with the
    padded size above, at and below n and n beyond one trip of 256 lanes; at 30 degrees the cap falls into many fans, whose
    count and order show in the points and faces"""
    v, f = S.cone(m, 0.4)
    rv, rf, holes, extra = _tail_equals_the_rules(v, f, 300.0)
    assert holes == 1 and np.bincount(rf.ravel())[m + 1] == m
    assert extra[(True, 30.0)] > m and extra[(False, 30.0)] == 0


def test_more_big_vertices_than_sort_workgroups(ivxlib):
    """513 cones over 49-gons: filled, 1026 vertices have 49 corners each -- more than the 1024 workgroups of k_fan_sort_big, whose
    loop over the list takes a second trip"""
    v, f = S.cones(513, 49)
    rv, rf, holes, extra = _tail_equals_the_rules(v, f, 300.0)
    assert holes == 513 and len(rf) == 50274
    assert (np.bincount(rf.ravel()) > S.FAN_LANE_MAX).sum() == 1026 > S.BIG_SORT_GRID
    assert extra[(True, 30.0)] > 513 * 49


def test_short_rims_and_a_single_triangle(ivxlib):
    """rims of 3, 4, 5, 7, 8 and 9 edges in one mesh (36 rim edges: cycle lengths on both sides of the powers of two of the pointer
    jumping), and the smallest mesh there is.  The capped triangle is flat, so auto-orientation goes by the sign of a volume that
    is zero in exact arithmetic -- but not an arbitrary one here: one point is the origin, three of the four terms a . (b x c) are
    exactly 0 on both sides, and the fourth (4.5e-9, from the float32 rounding of the centroid) is the whole sum in any order."""
    v, f = S.cones(6, [3, 4, 5, 7, 8, 9])
    assert _tail_equals_the_rules(v, f, 300.0)[2] == 6
    rv, rf, holes, _ = _tail_equals_the_rules(np.array([[0, 0, 0], [1, 0.1, 0], [0.2, 1, 0.3]], np.float32), np.array([[0, 1, 2]], np.int32), 300.0)
    assert holes == 1 and len(rf) == 4


def test_hole_of_exactly_the_hole_size_is_filled(ivxlib):
    v, f = S.pyramid_6x8()
    assert _tail_equals_the_rules(v, f, 5.0)[2] == 1
    assert _tail_equals_the_rules(v, f, float(np.nextafter(5.0, 0.0)))[2] == 0


@pytest.mark.parametrize("nt", [170, 171])
def test_edge_hash_at_its_smallest_table(ivxlib, nt):
    """510 directed edges fit the 1024-slot floor of the edge hash, 513 are the first to double it"""
    v, f = S.sheet(nt)
    assert _tail_equals_the_rules(v, f, 300.0)[2] == 1


# ---- geodesic graph builder --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 16, 17])
@pytest.mark.parametrize("name", ["closed", "open"])
def test_geodesic_graph_across_the_insertion_sort_limit(ivxlib, name, k):
    """the hub's raw neighbour list has 30 / 32 / 34 entries: insertion sort up to 32, heap sort past it"""
    from invesalius3_amd import polydata_utils as pu
    v, f, hub = S.FANS[name](k, 0, dtype=np.float32)
    m = pu.DeviceMesh.upload(v, f)
    off, adj = m.graph_arrays()
    woff, wadj = G.csr(f, len(v))
    assert np.array_equal(off, woff) and np.array_equal(adj, wadj)
    for s in (hub, int(f[0, 1])):
        d, pred, _ = m.geodesic_distances(s, with_stats=True)
        w = G.scipy_dijkstra(v, f, s)
        assert d.dtype == np.float64 and pred.dtype == np.int32 and np.array_equal(d, w)
        assert np.array_equal(pred == -1, ~np.isfinite(w) | (np.arange(len(v)) == s))
    m.close()


# ---- keep-largest ------------------------------------------------------------------------------------------------------------
def _keep_largest_equals_oracle(oracle, v, f):
    from invesalius3_amd import surface_process as sp
    v1, f1, nreg = sp.keep_largest(v, f)
    v0, f0, nreg0 = oracle.mesh_keep_largest(v, f)
    assert nreg == nreg0 and np.array_equal(f1, f0) and np.array_equal(v1.view(np.uint32), v0.view(np.uint32))
    return v0, f0, nreg0


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("sizes", [[1500, 1500, 600], [600, 1500, 1500]], ids=["tie-first", "tie-last"])
def test_region_split_between_hot_and_ballot_counting(ivxlib, oracle, sizes, order):
    """two regions of 1500 triangles tie and the first one wins; listed strip after strip, one of them has its triangles in two
    workgroups of k_mesh_tricount, counted as the workgroup's hot root in one and wave by wave in the other"""
    v, f, owner = S.strips(sizes, order)
    v0, f0, nreg = _keep_largest_equals_oracle(oracle, v, f)
    winner = sizes.index(1500) if order == "sorted" else int(owner[np.isin(owner, [i for i, n in enumerate(sizes) if n == 1500])][0])
    assert nreg == 3 and len(f0) == 1500 and np.array_equal(v0[f0], v[f[owner == winner]])


@pytest.mark.parametrize("sizes", [[1024, 1023], [1024, 1024], [1024, 1025]], ids=["2047", "2048-tie", "2049"])
def test_totals_at_the_counting_block_edge(ivxlib, oracle, sizes):
    v, f, owner = S.strips(sizes, "sorted")
    v0, f0, nreg = _keep_largest_equals_oracle(oracle, v, f)
    assert nreg == 2 and len(f0) == max(sizes) and np.array_equal(v0[f0], v[f[owner == (1 if sizes[1] > sizes[0] else 0)]])


@pytest.mark.parametrize("lead", [False, True], ids=["63-groups", "64-groups"])
def test_64_roots_in_every_wave(ivxlib, oracle, lead):
    """64 strips dealt in turn: every 64 consecutive triangles have 64 distinct roots.  As dealt, one of them is always the
    workgroup's hot root (triangles 0 and 2048 both open a turn), so the ballot loop of k_mesh_tricount peels 63 groups per wave;
    with one triangle of a region of its own listed first, the hot root of the first workgroup is that region and its waves 1 .. 31
    peel all 64"""
    v, f, owner = S.strips([40] * 64 + [41], "round_robin")
    if lead:
        v, f, owner = S.with_leading_triangle(v, f, owner)
    v0, f0, nreg = _keep_largest_equals_oracle(oracle, v, f)
    assert nreg == 65 + lead and len(f0) == 41 and np.array_equal(v0[f0], v[f[owner == 64]])


@pytest.mark.parametrize("big", S.SCAN_CASES)
def test_scans_at_the_block_edges(ivxlib, oracle, big):
    """a strip of `big` triangles next to one of 5: the scans of the keep flags and of the used points run over 4095 .. 4098 entries"""
    v, f, owner = S.strips([5, big], "sorted", spare=0)
    v0, f0, nreg = _keep_largest_equals_oracle(oracle, v, f)
    assert nreg == 2 and len(f0) == big and len(v0) == big + 2


def test_scan_carry_between_passes_of_the_block_sums(ivxlib, oracle):
    """4 198 401 points: the scan over the used points has 1026 block sums, two passes of k_mscan_sums.  The kept strip lies
    across element 4 194 304, so the new ids of its later points need the carry from the first pass to the second."""
    v, f = S.carry_strips()
    v0, f0, nreg = _keep_largest_equals_oracle(oracle, v, f)
    assert nreg == 2 and len(f0) == 2100 and len(v0) == 2102 and f0.max() == 2101


# ---- mass properties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 255, 1023, 1024, 1025, 262144, 262145])
def test_mass_sums_at_the_block_edges(ivxlib, oracle, nt):
    """soups and the same triangles indexed, with partial workgroups of k_mesh_mass and 256 | 257 partial records for the strided
    loop of k_mesh_mass_final.  The counters are exact.  The four sums: both sides add the SAME float64 terms (mass_terms; the host
    test checks them against the oracle's), the oracle with math.fsum, the kernels in a tree of at most 32 nested additions (4
    per lane, 6 + 2 across the workgroup, twice), each of which errs by at most 2^-53 of a partial sum of magnitudes: the
    difference is bounded by 32 * 2^-53 * sum |term|; 64 leaves a factor 2."""
    from invesalius3_amd import surface_process as sp
    tris = S.soup(nt, seed=nt)
    v, f = S.indexed(tris, seed=nt)
    area, div = S.mass_terms(tris)
    want = oracle.mesh_mass_properties(tris)
    assert oracle.mesh_mass_properties(v, f) == want
    for got in (sp.mass_properties_full(tris), sp.mass_properties_full(v, f)):
        assert got[5:] == want[5:]
        terms = [area, div[:, 0], div[:, 1], div[:, 2]]
        for q in range(4):
            bound = 64.0 * 2.0 ** -53 * math.fsum(np.abs(terms[q]))
            assert abs(got[1 + q] - want[1 + q]) <= bound, "nt %d sum %d: got %.17g want %.17g bound %.3g" % (nt, q, got[1 + q], want[1 + q], bound)
        kx, ky, kz = want[5:]
        assert got[0] == abs(kx * got[2] + ky * got[3] + kz * got[4])
