"""The cases of _mci_cases.py and the restatement _mci_ref.py, checked without a GPU: the restated constants are the ones the .hip /
.h text defines, every case sits on the word edge, pad combination or seam it is named for, and on every case the restated vertex
set is the set of distinct vertices of the C oracle's soup, bit for bit -- so the reference side of test_gpu_mci_edges.py is known
to be sound before a kernel runs."""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import _mci_cases as C
import _mci_ref as R
from _stitch_ref import stitch_piece_meshes
from conftest import synth_volume

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "invesalius3_amd", "csrc")
PIECES = C.piece_cases()
STITCHES = C.stitch_cases()


def _text(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _rows(v):
    """the distinct float32 triples of `v` by bit pattern, sorted"""
    return np.unique(np.ascontiguousarray(v, np.float32).reshape(-1, 3).view(np.uint32), axis=0)


def _tri_rows(soup):
    """the triangles (T, 3, 3) as sorted rows of nine bit patterns: the multiset"""
    t = np.ascontiguousarray(soup, np.float32).reshape(-1, 9).view(np.uint32)
    return t[np.lexsort(t.T[::-1])]


def test_constants_are_the_ones_the_sources_define():
    mci, common, scan = _text("k_mci.hip"), _text("mc_common.h"), _text("scan_u32.h")
    assert "g->ws = ivx::cdiv(g->nx, %d);" % C.WORD in common and "g->WX = ivx::cdiv(g->NX, %d);" % C.WORD in common
    assert "const int64_t rem = g.NX - ww * %d; // padded points in this word" % C.WORD in mci
    assert "const int64_t rem = g.NX - w * %d; " % C.WORD in mci and "const int64_t remx = g.NX - 1 - w * %d; " % C.WORD in mci
    assert "prev = t0 >> %d;" % (C.WORD - 1) in mci
    caps = re.findall(r"blocks < (\d+) \? blocks : (\d+)", mci)
    assert len(caps) >= 4 and all(int(a) == int(b) == C.GRID_CAP for a, b in caps)
    for kernel in ("k_mci_count", "k_mci_vertices", "k_mci_vertices_levels", "k_mci_faces"):
        assert "__launch_bounds__(256) void %s(" % kernel in mci
    assert "struct __attribute__((aligned(%d))) CrossRec {\n    uint64_t cx, cy, cz, cp;\n};" % C.CROSSREC_BYTES in mci
    assert C.CROSSREC_BYTES == 4 * 8
    m = re.findall(r"constexpr int MSCAN = (\d+);", scan)
    assert len(m) == 1 and 256 * int(m[0]) == C.SCAN_BLOCK
    assert "m.nsb = ivx::cdiv(m.npw, 256 * %d);" % (C.SCAN_BLOCK // 256) in mci
    # the order of a word's vertices, on both sides of the stitch
    assert "uint64_t m = ax == 0 ? c.cx : (ax == 1 ? c.cy : (ax == 2 ? c.cz : c.cp));" in mci


def test_every_case_sits_where_it_is_named():
    names = [c["name"] for c in PIECES]
    assert len(set(names)) == len(names)
    for c in PIECES:
        nz, ny, nx = c["array"].shape
        pxy = int(c["pad_xy"])
        assert c["NX"] == nx + 2 * pxy and c["NY"] == ny + 2 * pxy and c["NZ"] == nz + int(c["pad_bottom"]) + int(c["pad_top"])
        assert c["WX"] == (c["NX"] + 63) // 64 and c["ws"] == (nx + 63) // 64
        if "want_NX" in c:
            assert c["NX"] == c["want_NX"], c["name"]
    ints = [c for c in PIECES if c["group"] == "ints"]
    assert {(c["NX"], (c["pad_xy"], c["pad_bottom"], c["pad_top"])) for c in ints} >= {(n, p) for n in C.WORD_EDGE_NX for p in C.PADS3}
    assert {(c["pad_xy"], c["pad_bottom"], c["pad_top"], c["vtk_pz"]) for c in ints if c["NX"] == 65} == {
        (a, b, t, z) for a in (False, True) for b in (False, True) for t in (False, True) for z in (0, 1)}
    # the padded row is one bit ahead of the source row: both "one word more than the source" and "as many" occur, at a whole
    # word, a partial word and a word with one point
    assert {(c["NX"] % 64, c["WX"] - c["ws"]) for c in ints} >= {(63, 0), (0, 0), (1, 0), (1, 1)}
    assert {c["NX"] for c in PIECES if c["group"] in ("pad_on_iso", "pad_inside")} == {64, 65}
    assert {c["pad_value"] for c in PIECES if c["group"] == "pad_on_iso"} == {2.0}
    assert all(c["pad_value"] > c["iso_values"][0] for c in PIECES if c["group"] == "pad_inside")
    assert {(c["NX"], c["pad_xy"]) for c in PIECES if c["group"] == "u16"} == {(65, True), (128, False)}
    assert all(c["array"].dtype == np.uint16 and (c["array"] == 40000).any() for c in PIECES if c["group"] == "u16")
    big = C.by_name("past_scan_block")
    assert big["NZ"] * big["NY"] * big["WX"] == 32 * 42 * 4 > C.SCAN_BLOCK


def test_planted_samples_sit_on_the_seams_with_one_crossing_from_the_named_side():
    planted = [c for c in PIECES if c["group"] == "planted"]
    seen = set()
    for c in planted:
        P = R.padded_grid(c["array"], False, False, False, 0.0)
        S, E, cross, point = R.crossing_planes(P, 5.0)
        k, jf, i = c["point"]
        assert np.argwhere(E).tolist() == [[k, jf, i]] and np.argwhere(point).tolist() == [[k, jf, i]]
        assert np.argwhere(~S).tolist() == [list(c["neighbour"])]
        # the crossings that leave or reach the point, by direction: only the named one
        found = []
        for d, (dk, dj, di) in C.DIRECTIONS.items():
            q = (k + dk, jf + dj, i + di)
            if all(0 <= v < n for v, n in zip(q, P.shape)) and S[q] != S[k, jf, i]:
                found.append(d)
        assert found == [c["direction"]], c["name"]
        seen.add((i & 63, c["direction"]))
    for d in C.DIRECTIONS:  # bit 0 and bit 63 of a word, every direction; "-x" at bit 0 of word 1 reads the word before
        assert (0, d) in seen and (63, d) in seen
    assert any(c["point"][2] == 64 and c["direction"] == "-x" for c in planted)
    assert any(c["point"][2] == 63 and c["direction"] == "+x" for c in planted)
    assert any(c["interior"] for c in planted) and any(not c["interior"] for c in planted)


@pytest.mark.parametrize("group", ["ints", "planted", "pad_on_iso", "pad_inside", "u16", "thin", "past_scan_block"])
def test_restated_vertices_are_the_distinct_vertices_of_the_oracle_soup(oracle, group):
    cases = [c for c in PIECES if c["group"] == group]
    assert cases
    for c in cases:
        a = c["array"]
        soups = []
        for iso in c["iso_values"]:
            soup = oracle.marching_cubes(a, *C.args_of(c, [iso]))
            verts, keys = R.indexed_vertices(a, c["spacing"], iso, *C.args_of(c)[2:])
            assert verts.dtype == np.float32 and verts.shape == (len(keys), 3) and keys.shape == (len(keys), 5), c["name"]
            # no vertex twice (lookup raises), every corner of the soup among them (it raises), and every one of them a corner
            at = R.lookup(verts, soup.reshape(-1, 3))
            assert len(np.unique(at)) == len(verts), c["name"]
            assert np.array_equal(verts[at].view(np.uint32), soup.reshape(-1, 3).view(np.uint32)), c["name"]
            # sorted by key, and no key twice
            if len(keys) > 1:
                order = np.lexsort(tuple(keys[:, q] for q in (4, 3, 2, 1, 0)))
                assert np.array_equal(order, np.arange(len(keys))) and (np.diff(keys, axis=0) != 0).any(axis=1).all()
            soups.append(soup)
            if c["group"] == "planted" and c["interior"]:
                assert len(soup) == 8 and len(verts) == 6 and int((keys[:, 3] == R.KIND_POINT).sum()) == 1, c["name"]
            if c["group"] == "planted":
                assert int((keys[:, 3] == R.KIND_POINT).sum()) == 1 and tuple(keys[keys[:, 3] == 3][0, [0, 1]]) == c["point"][:2]
            if c.get("empty"):
                assert len(soup) == 0 and len(verts) == 0
        whole = oracle.marching_cubes(a, *C.args_of(c))
        assert np.array_equal(whole, np.concatenate(soups)), c["name"]  # the two iso-values' triangles follow each other
        if group == "past_scan_block":
            continue
        v, f = R.indexed_mesh(a, C.args_of(c), soups)
        assert f.dtype == np.int32 and np.array_equal(v[f].view(np.uint32).reshape(-1, 3, 3), whole.view(np.uint32)), c["name"]
    if group in ("ints", "pad_on_iso", "pad_inside", "u16", "past_scan_block"):  # they do exercise point vertices
        c = cases[0]
        _, keys = R.indexed_vertices(c["array"], c["spacing"], c["iso_values"][0], *C.args_of(c)[2:])
        assert (keys[:, 3] == R.KIND_POINT).any()


def test_stitch_pieces_restate_the_slab_layout():
    from invesalius3_amd import parallel as par
    for c in STITCHES:
        for rank in range(c["world"]):
            lay = par.slab_layout(rank, c["world"], c["nz"])
            m = par.slab_mc_args(lay, c["fill_border_holes"])
            a, args = C.stitch_piece(c, rank)
            lo = lay.z_global0 - lay.hb  # the rank's stored slices begin here
            assert np.array_equal(a, c["whole"][lo + m["z0"]:lo + m["z1"]])
            fbh = c["fill_border_holes"]
            assert args[2:] == (m["roi_start"], fbh, bool(m["pad_bottom"]), bool(m["pad_top"]), c["pad_value"], int(bool(m["pad_bottom"])))


@pytest.mark.parametrize("name", [c["name"] for c in STITCHES])
def test_float_stitch_of_restated_pieces_is_the_whole_volume_mesh(oracle, name):
    c = [s for s in STITCHES if s["name"] == name][0]
    if "want_NX" in c:
        assert c["whole"].shape[2] + 2 * int(c["fill_border_holes"]) == c["want_NX"]
    pieces, keys, NZs = [], [], []
    for rank in range(c["world"]):
        a, args = C.stitch_piece(c, rank)
        pieces.append(R.indexed_mesh(a, args, oracle.marching_cubes(a, *args)))
        keys.append(R.indexed_vertices(a, args[0], args[1][0], *args[2:])[1])
        NZs.append(C.geometry(a.shape, *args[3:6])[0])
    # (with the planted neighbour below or above the shared plane, the whole surface lies in one rank: the other has none)
    assert sum(len(p[1]) > 0 for p in pieces) == (1 if c.get("want_dropped") == 0 else c["world"])
    sv, sf = stitch_piece_meshes(pieces)
    wargs = C.stitch_whole_args(c)
    wsoup = oracle.marching_cubes(c["whole"], *wargs)
    wv, wf = R.indexed_mesh(c["whole"], wargs, wsoup)
    assert not R.has_duplicates(sv) and np.array_equal(_rows(sv), _rows(wv)) and len(sv) == len(wv)
    assert np.array_equal(_tri_rows(sv[sf]), _tri_rows(wsoup))
    shared = [R.shared_plane_counts(keys[r - 1], keys[r], NZs[r - 1]) for r in range(1, c["world"])]
    assert sum(len(p[0]) for p in pieces) - len(sv) == sum(shared)
    if "want_dropped" in c:
        assert shared == [c["want_dropped"]]
        on_iso = keys[0][(keys[0][:, 3] == R.KIND_POINT)]
        # the on-iso sample lies on the shared plane; the lower piece sees its crossing unless the neighbour is above
        assert (len(on_iso) == 1 and tuple(on_iso[0][:2]) == (3, 2)) == (c["direction"] != "+z")
    else:
        assert all(s > 0 for s in shared)
    if c["name"].startswith("stitch_int16") or c["name"].startswith("stitch_uint16"):  # on-iso samples on the shared planes
        assert any(((k[:, 0] == 0) & (k[:, 3] == R.KIND_POINT)).any() for k in keys[1:])


def test_levels_volumes_grow_across_the_word_seam():
    for dx in C.LEVELS_DX:
        img = synth_volume((6, 9, dx), seed=C.LEVELS_SEED)
        mask = (img >= C.LEVELS_THRESHOLD[0]) & (img <= C.LEVELS_THRESHOLD[1])
        grow = (img >= C.LEVELS_GROW[0]) & (img <= C.LEVELS_GROW[1])
        z, y, x = (int(v[0]) for v in np.nonzero(grow))
        lab, _ = ndimage.label(grow, np.ones((3, 3, 3)))
        comp = lab == lab[z, y, x]
        assert (mask & ~comp).any() and (~mask).any()  # three byte levels: 0, 255 and 254
        reach = comp.any(axis=(0, 1))
        assert reach[min(63, dx - 1)] and reach[dx - 1] and (dx <= 64 or reach[64])
