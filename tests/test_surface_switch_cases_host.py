"""The cases of _surface_switch_cases.py, checked without a GPU: the restated constants are the ones the .hip / .h text defines (a
retune fails here instead of moving a case off its switch unnoticed), every case stands on the side of its switch that it is
named for -- counted on the references alone -- and the two inputs that are meant to show an ORDER do show it on the reference.
The GPU half is test_gpu_surface_switches.py."""
import os
import re

import numpy as np
import pytest

import _geodesic_ref as G
import _mesh_tail_ref as ref
import _surface_switch_cases as S

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "invesalius3_amd", "csrc")
OPTS = (0.7, 3.0, 0.5, 10)


def _text(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]


def _body(text, kernel):
    """the text of one kernel / function: from its name to the next line that starts a definition"""
    at = text.index(kernel + "(")
    end = re.search(r"\n(?:__global__|__device__|static|constexpr|struct|template|extern|\})", text[at:])
    return text[at:at + end.start()] if end else text[at:]


# ---- the constants ----
def test_constants_are_the_ones_the_sources_define():
    smooth, tail, geo, mesh = _text("k_smooth.hip"), _text("k_meshtail.hip"), _text("k_meshgeo.hip"), _text("k_mesh.hip")
    regions, scan = _text("mesh_regions.h"), _text("scan_u32.h")
    assert int(_one(r"constexpr int RL = (\d+);", smooth)) == S.RL
    assert "if (len <= (uint32_t)RL) {" in smooth and "if (n >= (uint32_t)RL) out[n] = vj;" in smooth
    assert int(_one(r"constexpr uint32_t FAN_LANE_MAX = (\d+);", tail)) == S.FAN_LANE_MAX
    assert "if (n > FAN_LANE_MAX) {" in tail
    assert int(_one(r"for \(int step = 0; step < (\d+); step\+\+\)", _body(tail, "void k_rim_next"))) == S.RIM_TURNS
    assert int(_one(r"std::min<int64_t>\(ne / FAN_LANE_MAX \+ 1, (\d+)\)", tail)) == S.BIG_SORT_GRID
    hs = _body(tail, "uint32_t hash_slots")
    assert int(_one(r"uint64_t m = (\d+);", hs)) == S.HASH_MIN_SLOTS and "while (m < (uint64_t)ne * 2u) m <<= 1;" in hs
    assert "!(radius > hole_size)" in tail
    assert int(_one(r"if \(n <= (\d+)u\) \{", _body(geo, "void k_geo_sort_unique"))) == S.GEO_INSERTION_MAX
    tc = _body(regions, "void k_mesh_tricount")
    assert 256 * int(_one(r"constexpr int TPL = (\d+);", regions)) == S.TRICOUNT_BLOCK
    assert "blockIdx.x * 256 * TPL" in tc and "__launch_bounds__(256) void k_mesh_tricount" in regions
    assert "ivx::cdiv(ntris, 256 * TPL)" in mesh
    assert 256 * int(_one(r"constexpr int MASS_TPL = (\d+);", mesh)) == S.MASS_BLOCK
    assert "ivx::cdiv(ntris, 256 * MASS_TPL)" in mesh and "__launch_bounds__(256) void k_mesh_mass(" in mesh
    assert int(_one(r"for \(int64_t b = threadIdx\.x; b < nb; b \+= (\d+)\)", _body(mesh, "void k_mesh_mass_final"))) == S.MASS_FINAL_LANES
    assert 256 * int(_one(r"constexpr int MSCAN = (\d+);", scan)) == S.SCAN_BLOCK
    assert "ivx::cdiv(n, 256 * MSCAN)" in scan and "__launch_bounds__(256) void k_mscan_block" in scan
    sums = _body(scan, "void k_mscan_sums")
    assert int(_one(r"for \(int64_t b0 = 0; b0 < nb; b0 \+= (\d+)\)", sums)) == S.SCAN_SUMS_PASS
    assert "__launch_bounds__(%d) void k_mscan_sums" % S.SCAN_SUMS_PASS in scan
    # the statement of the rules in Python turns through as many faces as the kernel
    with open(ref.__file__) as fh:
        assert int(_one(r"for _ in range\((\d+)\):  # turn about the end point", fh.read())) == S.RIM_TURNS


# ---- smoothing: the fans ----
def _hub_counts(oracle, v, f, hub):
    """(entries in the hub's incident-face list, its unique neighbours).  A face that names the hub twice is listed twice, as
    k_sm_count files it; the neighbours are the reference's own (build_vertex_connectivity)."""
    off, idx = oracle.mesh_vertex_connectivity(f, len(v))
    nb = idx[off[hub]:off[hub + 1]]
    assert len(set(nb.tolist())) == len(nb)
    return int(np.bincount(f.ravel(), minlength=len(v))[hub]), len(nb)


def _path(entries, neighbours):
    if entries > S.RL:
        return "sort-in-place"
    return "mixed" if neighbours > S.RL else "registers"


@pytest.mark.parametrize("hub_id", S.HUB_IDS)
def test_fan_ladder_stands_on_both_sides_of_RL(oracle, hub_id):
    seen = {}
    for name, k in S.FAN_LADDER:
        v, f, hub = S.FANS[name](k, hub_id)
        assert hub == (len(v) - 1 if hub_id == "last" else hub_id) and f.dtype == np.int32 and f.max() == len(v) - 1
        want = {"closed": (k, k), "open": (k, k + 1), "bowtie": (k, 2 * k)}[name]
        assert _hub_counts(oracle, v, f, hub) == want
        seen[(name, k)] = _path(*want)
        for kind, more in (("degenerate", 2), ("duplicate", 1)):
            v2, f2, _ = S.with_repeat(v, f, hub, kind)
            assert _hub_counts(oracle, v2, f2, hub) == (want[0] + more, want[1])
            seen[(name, k, kind)] = _path(want[0] + more, want[1])
        # no other vertex of a fan comes near the switch
        assert np.delete(np.bincount(f.ravel(), minlength=len(v)), hub).max() <= 2
    assert [seen[("closed", k)] for k in (11, 12, 13)] == ["registers", "registers", "sort-in-place"]
    assert [seen[("open", k)] for k in (11, 12, 13)] == ["registers", "mixed", "sort-in-place"]
    assert [seen[("bowtie", k)] for k in (6, 7, 11, 12, 13)] == ["registers", "mixed", "mixed", "mixed", "sort-in-place"]
    assert S.RL == 12  # bowtie(6): exactly RL neighbours; bowtie(12): RL faces and 2 RL neighbours, the padded list brim-full
    # a repeated face is met by the register sort and by the in-place sort, right at the switch
    assert seen[("closed", 11, "duplicate")] == "registers" and seen[("closed", 12, "duplicate")] == "sort-in-place"
    assert seen[("bowtie", 6, "degenerate")] == "registers" and seen[("bowtie", 7, "degenerate")] == "mixed"
    assert seen[("closed", 11, "degenerate")] == "sort-in-place"


@pytest.mark.parametrize("hub_id", S.HUB_IDS)
@pytest.mark.parametrize("name,k", S.FAN_LADDER + [("closed", 40)])  # (40: the fan of test_gpu_smooth.py, seed 2)
def test_float64_fans_show_the_neighbour_order(oracle, name, k, hub_id):
    """the condition the float32 fan of test_gpu_smooth.py does not meet: with the face list reversed -- the hub's neighbours in
    the opposite order -- the reference moves the hub somewhere else"""
    v, f, hub = S.FANS[name](k, hub_id, seed=2 if k == 40 else 0, dtype=np.float64)
    out = []
    for faces in (f, S.reversed_faces(f)):
        p = v.copy()
        flags, w = oracle.context_aware_smoothing(p, S.faces4(faces), oracle.mesh_face_normals(v, faces), *OPTS, details=True)
        assert flags.all() and (w == 1.0).all()  # (Q-M2: every vertex of a face is a seed)
        out.append(p)
    assert not np.array_equal(out[0][hub], out[1][hub]), (name, k, hub_id)
    assert np.abs(out[0] - out[1]).max() < 1e-12  # the same smoothing, to rounding


@pytest.mark.parametrize("side", ["far", "near"])
def test_tie_strip_shows_which_seed_won(oracle, side):
    v, f, seeds, info = S.tie_strip(side)
    left, right = info["seeds"]
    assert (left < right) == (side == "far") and v[left, 0] == -2.0 and v[right, 0] == 2.0
    mirror = v * np.array([-1.0, 1.0, 1.0])
    strip = [i for i in range(len(v)) if i not in info["dangling"]]
    assert {tuple(p) for p in v[strip].tolist()} == {tuple(p) for p in mirror[strip].tolist()}  # the strip is its own mirror image
    assert (v[list(info["dangling"]), 0] > 0).all() and np.array_equal(v * 4, np.round(v * 4))
    tmax, bmin = 10.0, 0.5
    w = oracle.mesh_propagate_weights(v, f, seeds, tmax, bmin)
    d2 = lambda a, b: float(((v[a] - v[b]) ** 2).sum())
    assert d2(info["mid"], left) == d2(info["mid"], right) == 4.0 and w[info["mid"]] == S.weight_of(4.0, tmax, bmin)
    for d in info["dangling"]:
        cand = {s: S.weight_of(d2(d, s), tmax, bmin) for s in (left, right)}
        assert cand[left] != cand[right]
        assert w[d] == cand[min(left, right)]
    # float32 positions hold the same numbers
    assert np.array_equal(oracle.mesh_propagate_weights(v.astype(np.float32), f, seeds, tmax, bmin), w)


def test_edge_345_is_in_at_5_and_out_just_below(oracle):
    v, f, seeds, ids = S.edge_345()
    assert float((v[ids["P"]] ** 2).sum()) == 25.0 == 5.0 * 5.0
    w = oracle.mesh_propagate_weights(v, f, seeds, 5.0, 0.5)
    assert w[ids["S"]] == 1.0 and w[ids["P"]] == 0.5 == w[ids["Q"]] and w[ids["C"]] > 0.5 and w[ids["E"]] > 0.5
    below = float(np.nextafter(5.0, 0.0))
    assert below * below < 25.0
    w = oracle.mesh_propagate_weights(v, f, seeds, below, 0.5)
    assert w.tolist() == [1.0, 0.5, 0.5, 0.5, 0.5]


def test_strip_300_takes_many_rounds():
    v, f = G.strip(300)
    off, adj = G.csr(f, len(v))
    hops = np.full(len(v), -1)
    hops[0], front = 0, [0]
    while front:
        nxt = []
        for a in front:
            for b in adj[off[a]:off[a + 1]].tolist():
                if hops[b] < 0:
                    hops[b] = hops[a] + 1
                    nxt.append(b)
        front = nxt
    assert hops.max() >= 149  # rounds of the relaxation: one per hop from the seed (today's meshes end within ten)


# ---- hole filling and point normals ----
def _corners(faces, nv):
    return np.bincount(np.asarray(faces).ravel(), minlength=nv)


@pytest.mark.parametrize("k", [3, S.RIM_TURNS - 1, S.RIM_TURNS, S.RIM_TURNS + 1])
def test_open_fan_rim_closes_up_to_64_faces_at_the_hub(k):
    v, f, hub = S.open_fan(k, 0, dtype=np.float32)
    assert _corners(f, len(v))[hub] == k and len(ref.boundary_edges(f)) == k + 2
    fv, ff, holes = ref.fill_holes(v, f, 300.0)
    if k <= S.RIM_TURNS:
        assert holes == 1 and len(ff) == len(f) + k + 2 and _corners(ff, len(fv))[hub] == k + 2
        assert len(ref.boundary_edges(ff)) == 0
    else:
        assert holes == 0 and np.array_equal(ff, f)
    if k >= S.RIM_TURNS - 1:
        assert _corners(ff, len(fv))[hub] > S.FAN_LANE_MAX


CONE_M = [47, 48, 49, 64, 65, 255, 256, 257, 300]


@pytest.mark.parametrize("m", CONE_M)
def test_cone_centroid_has_m_corners_and_the_cap_falls_apart(m):
    v, f = S.cone(m, 0.4)
    fv, ff, holes = ref.fill_holes(v, f, 300.0)
    assert holes == 1 and len(fv) == m + 2 and len(ff) == 2 * m
    c = _corners(ff, len(fv))
    assert c[0] == m and c[m + 1] == m and c[1:m + 1].max() == 4  # apex and centroid: m corners each
    assert (m > S.FAN_LANE_MAX) == (m >= 49)
    pad = 1 << (m - 1).bit_length()
    assert {47: 64, 48: 64, 49: 64, 64: 64, 65: 128, 255: 256, 256: 256, 257: 512, 300: 512}[m] == pad
    ov, of, _, _ = ref.point_normals(fv, ff, 30.0, True, True)
    fans = int((ov == fv[m + 1]).all(axis=1).sum())  # the centroid and its copies: one point per fan
    assert len(ov) - len(fv) > m and fans > m // 2  # many extra points, and the centroid alone is in many fans


def test_many_cones_give_more_big_vertices_than_the_grid_has_workgroups():
    v, f = S.cones(513, 49)
    assert len(f) == 513 * 49 and len(v) == 513 * 50
    c = _corners(f, len(v))
    assert (c > S.FAN_LANE_MAX).sum() == 513  # the apexes; filled, the 513 centroids join them (checked on one cone above)
    assert 2 * 513 > S.BIG_SORT_GRID and 2 * len(f) == 50274


def test_short_rims_and_the_hash_floor():
    v, f = S.cones(6, [3, 4, 5, 7, 8, 9])
    loops = ref.rim_loops(f)
    assert sorted(len(l) for l in loops) == [3, 4, 5, 7, 8, 9] and sum(len(l) for l in loops) == 36
    fv, ff, holes = ref.fill_holes(v, f, 300.0)
    assert holes == 6 and len(ref.boundary_edges(ff)) == 0
    fv, ff, holes = ref.fill_holes(np.eye(3, dtype=np.float32), np.array([[0, 1, 2]], np.int32), 300.0)
    assert holes == 1 and len(ff) == 4
    for nt in (170, 171):
        v, f = S.sheet(nt)
        assert len(f) == nt and len(ref.rim_loops(f)) == 1 and len(ref.boundary_edges(f)) == nt + 2
        slots = S.HASH_MIN_SLOTS
        while slots < 2 * 3 * nt:
            slots *= 2
        assert slots == (S.HASH_MIN_SLOTS if nt == 170 else 2 * S.HASH_MIN_SLOTS)


def test_pyramid_rim_radius_is_exactly_5():
    v, f = S.pyramid_6x8()
    assert ref.fill_holes(v, f, 5.0)[2] == 1
    assert ref.fill_holes(v, f, float(np.nextafter(5.0, 0.0)))[2] == 0


# ---- geodesic graph ----
@pytest.mark.parametrize("k", [15, 16, 17])
def test_geodesic_fans_have_raw_lists_of_30_32_34(k):
    for build in (S.closed_fan, S.open_fan):
        v, f, hub = build(k, 0, dtype=np.float32)
        raw = 2 * _corners(f, len(v))  # two entries per triangle at the point
        assert raw[hub] == 2 * k and np.delete(raw, hub).max() <= 4
    assert (2 * 15 < S.GEO_INSERTION_MAX) and 2 * 16 == S.GEO_INSERTION_MAX and 2 * 17 > S.GEO_INSERTION_MAX


# ---- keep-largest ----
def _per_block(owner, nreg):
    """triangles of every strip in every block of TRICOUNT_BLOCK consecutive triangles: (blocks, strips)"""
    nb = -(-len(owner) // S.TRICOUNT_BLOCK)
    out = np.zeros((nb, nreg), np.int64)
    np.add.at(out, (np.arange(len(owner)) // S.TRICOUNT_BLOCK, owner), 1)
    return out


def test_strips_split_regions_between_the_two_counting_paths():
    v, f, owner = S.strips([1500, 1500, 600], "sorted")
    pb = _per_block(owner, 3)
    assert pb.tolist() == [[1500, 548, 0], [0, 952, 600]]
    # the workgroup's first triangle names its hot region: strip 1 is counted by the ballot path in block 0, as the hot one in block 1
    assert owner[0] == 0 and owner[S.TRICOUNT_BLOCK] == 1
    v, f, owner = S.strips([600, 1500, 1500], "sorted")
    assert _per_block(owner, 3).tolist() == [[600, 1448, 0], [0, 52, 1500]] and owner[S.TRICOUNT_BLOCK] == 1
    v, f, owner = S.strips([1500, 1500, 600], "shuffled")
    assert (_per_block(owner, 3) > 0).all()
    for total, sizes in ((2047, [1024, 1023]), (2048, [1024, 1024]), (2049, [1024, 1025])):
        assert sum(sizes) == total and S.TRICOUNT_BLOCK == 2048
    v, f, owner = S.strips([1024, 1025], "sorted")
    assert _per_block(owner, 2).tolist() == [[1024, 1024], [0, 1]]


def test_round_robin_puts_64_roots_into_every_wave():
    sizes = [40] * 64 + [41]
    v, f, owner = S.strips(sizes, "round_robin")
    assert len(f) == 64 * 40 + 41 and np.bincount(owner).tolist() == sizes
    for w in range(40):
        assert sorted(owner[64 * w:64 * w + 64].tolist()) == list(range(64))
    assert (owner[64 * 40:] == 64).all()
    # the hot root of a workgroup is the region of its first triangle: strip 0 in both, which every wave holds -- 63 other roots
    assert owner[0] == 0 and owner[S.TRICOUNT_BLOCK] == 0
    v2, f2, owner2 = S.with_leading_triangle(v, f, owner)
    assert owner2[0] == 65 and (owner2[1:] == owner).all() and np.array_equal(f2[1:], f) and f2[0].min() == len(v)
    for w in range(1, S.TRICOUNT_BLOCK // 64):  # first workgroup, every wave but the first: 64 roots, none of them the hot one
        assert sorted(owner2[64 * w:64 * w + 64].tolist()) == list(range(64))
    # every strip really is one region of its own
    lab = G.edges(f)
    parent = np.arange(len(v))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for a, b in lab.tolist():
        ra, rb = find(a), find(b)
        parent[max(ra, rb)] = min(ra, rb)
    assert len({find(int(t[0])) for t in f}) == 65


def test_scan_cases_stand_on_the_block_edges():
    keep_n, used_n = [], []
    for big in S.SCAN_CASES:
        v, f, owner = S.strips([5, big], "sorted", spare=0)
        keep_n.append(len(f) + 1)  # the scan over the kept triangles runs over ntris + 1 entries
        used_n.append(len(v) + 1)  # ... and the one over the used points over nverts + 1
        assert len(f) == big + 5 and len(v) == big + 9
    edge = [S.SCAN_BLOCK - 1, S.SCAN_BLOCK, S.SCAN_BLOCK + 1]
    assert set(edge) <= set(keep_n) and set(edge + [S.SCAN_BLOCK + 2]) <= set(used_n)
    v, f = S.carry_strips()
    assert len(v) == 4198401 and len(v) + 1 > S.SCAN_SUMS_PASS * S.SCAN_BLOCK
    big = f[40:]
    assert big.min() < S.SCAN_SUMS_PASS * S.SCAN_BLOCK < big.max() and len(big) > len(f) - len(big)


# ---- mass properties ----
def test_mass_terms_are_the_oracles_terms(oracle):
    import math
    for nt in (1, 255, 1025):
        t = S.soup(nt, seed=nt)
        area, div = S.mass_terms(t)
        want = oracle.mesh_mass_properties(t)
        assert want[1] == math.fsum(area) and [want[2], want[3], want[4]] == [math.fsum(div[:, q]) for q in range(3)]
        v, f = S.indexed(t, seed=nt)
        assert np.array_equal(v[f], t)
        a2, d2 = S.mass_terms(v, f)
        assert np.array_equal(a2, area) and np.array_equal(d2, div)
        # well shaped: no sliver whose cross product cancels
        e = np.linalg.norm(t - np.roll(t, 1, axis=1), axis=2)
        assert e.min() > 0.4 and e.max() < 1.8 and area.min() > 0.05
    for nt, nb in ((1023, 1), (1024, 1), (1025, 2), (262144, 256), (262145, 257)):
        assert -(-nt // S.MASS_BLOCK) == nb
    assert 256 == S.MASS_FINAL_LANES < 257
