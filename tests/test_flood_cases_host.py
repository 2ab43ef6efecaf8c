"""CPU: the cases of tests/_flood_cases.py are what they claim to be, before the GPU is asked (tests/test_gpu_flood_coarse.py).

For every case: the C oracle's floodfill_threshold equals the seed components of scipy.ndimage.label on
(t0 <= img <= t1) & (out != fill); the construction facts hold (which bodies a flood joins under 6 / 18 / 26, how many blocks
are all-candidate, how many tile hops a path has); and ivx_flood_describe -- the engine's own host-side decisions, no device
call -- puts the case's shape on the path it was built for.  A table pins ivx_flood_describe at the edges that follow from
the constants of csrc/k_flood.hip."""
import ctypes

import numpy as np
import pytest

import _flood_cases as fc


@pytest.fixture(scope="module")
def describe():
    from invesalius3_amd import _lib, build

    lib = ctypes.CDLL(build.build())
    lib.ivx_flood_describe.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.ivx_flood_describe.restype = ctypes.c_int
    lib.ivx_flood_strct_bits.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def run(shape, nseeds, strct=None):
        s3 = np.ascontiguousarray(fc.structure(3) if strct is None else strct, dtype=np.uint8)
        bits = ctypes.c_uint32(0)
        assert lib.ivx_flood_strct_bits(_lib.ptr(s3), _lib.i64(s3.shape), ctypes.byref(bits)) == 0
        dz, dy, dx = shape
        plan = _lib.FloodPlan(dz, dy, dx, -(-dx // 64), bits.value)
        out = (ctypes.c_int32 * 8)()
        assert lib.ivx_flood_describe(ctypes.byref(plan), nseeds, out) == 0
        return list(out)

    return run


ON, BLOCK, PER_TILE, LANES, ROWS_PER_LANE, FUSED, GRID_CAP, TILES = range(8)


# ---- the edge table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx,on,block", [(1024, 1, 16), (1025, 1, 32), (2048, 1, 32), (2049, 1, 64), (4096, 1, 64),
                                         (4097, 0, 0)])
def test_describe_block_width_edges(describe, dx, on, block):
    d = describe((18, 35, dx), 1)
    assert (d[ON], d[BLOCK], d[PER_TILE]) == (on, block, 64 // block if block else 0)
    assert d[FUSED] == on                                 # no coarse pass, no fused start
    assert d[TILES] == -(-dx // 64) * 3 * 2 and d[GRID_CAP] == min(d[TILES], 1536)


@pytest.mark.parametrize("nty,ntz,lanes,per_lane", [(8, 8, 64, 1), (13, 5, 128, 1), (32, 32, 1024, 1), (41, 25, 1024, 2),
                                                    (86, 85, 1024, 8)])
def test_describe_lanes_and_rows_per_lane_edges(describe, nty, ntz, lanes, per_lane):
    d = describe((ntz * 16 - 5, nty * 16, 3), 1)
    assert (d[ON], d[LANES], d[ROWS_PER_LANE]) == (1, lanes, per_lane)


def test_describe_lds_limit_edge(describe):
    assert describe((85 * 16, 86 * 16, 3), 1)[ON] == 1    # 88 * 87 = 7656 halo rows
    assert describe((86 * 16, 86 * 16, 3), 1)[:6] == [0, 0, 0, 0, 0, 0]  # 88 * 88 = 7744 > 7680
    assert describe((16, 2558 * 16, 3), 1)[ON] == 1       # (2558 + 2) * 3 = 7680
    assert describe((16, 2559 * 16, 3), 1)[ON] == 0


@pytest.mark.parametrize("nseeds,fused", [(0, 0), (1, 1), (16, 1), (17, 0), (5000, 0)])
def test_describe_fused_start_edges(describe, nseeds, fused):
    assert describe((18, 35, 1100), nseeds)[FUSED] == fused


def test_describe_round_grid_cap_and_generic_structure(describe):
    assert describe((2, 800, 3300), 5000)[GRID_CAP:] == [1536, 2600]
    assert describe((16, 16 * 24, 64 * 64), 1)[GRID_CAP:] == [1536, 1536]
    assert describe((16, 16 * 24, 64 * 64 - 64), 1)[GRID_CAP:] == [1512, 1512]
    s = fc.structure(1).copy()
    s[1, ::2, ::2] = True                                  # none of the three standard structures: rounds only
    assert describe((18, 35, 1100), 1, s)[:6] == [0, 0, 0, 0, 0, 0]
    for conn in (1, 2, 3):
        assert describe((18, 35, 1100), 1, fc.structure(conn))[:6] == [1, 32, 2, 64, 1, 1]


def test_expected_path_restates_the_engine(describe):
    """the constants restated in _flood_cases.py against the engine's, on every shape the cases use and around the limits"""
    shapes = [fc.widths_case(dx).shape for dx in fc.WIDTHS] + [(n * 16 - 5, m * 16 - 7, dx) for m, n, dx in fc.ROWS.values()]
    shapes += [(1, 944, 1100), (2, 800, 3300), (2, 3, 1925), (16, 16 * 64, 5), (16, 16 * 65, 5), (512, 512, 512)]
    for shape in shapes:
        for nseeds in (1, 16, 17):
            assert describe(shape, nseeds) == fc.expected_path(shape, nseeds), (shape, nseeds)


# ---- (a) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx", fc.WIDTHS)
def test_widths_cases_are_on_their_path(describe, dx):
    case = fc.widths_case(dx)
    b = {1024: 16, 1025: 32, 1100: 32, 2048: 32, 2049: 64, 2500: 64, 4096: 64, 4097: 0}[dx]
    one, many = describe(case.shape, 1), describe(case.shape, 17)
    assert (one[ON], one[BLOCK], one[FUSED], many[FUSED]) == (int(b > 0), b, int(b > 0), 0)
    assert case.facts["block"] == (b or 64)
    assert [len(s) for _, s, _ in case.floods] == [1, 1, 17, 4]
    # the share of blocks that are all-candidate: exactly the bodies' blocks, as built (the loose voxels make none)
    whole, exist = fc.whole_block_share(case, 1)
    assert whole == case.facts["whole_blocks"] and 0.02 < whole / exist < 0.5
    assert 0.025 < case.facts["loose_share"] < 0.031     # of the voxels outside the bodies and the zones kept empty
    # the first seed sits in a whole block, the second in a block that is not
    bw = case.facts["block"]
    c = (case.img == fc.VAL) & (case.out0 != 1)
    for (name, seeds, _), want in zip(case.floods[:2], (True, False)):
        x, y, z = seeds[0]
        blk = c[z // 16 * 16:z // 16 * 16 + 16, y // 16 * 16:y // 16 * 16 + 16, x // bw * bw:x // bw * bw + bw]
        assert bool(blk.all()) == want, name
    # G | H: one block without a candidate;  G2 | H2: one such plane;  E stops one voxel short of its block
    g, h, g2, h2, e = (case.bodies[k][2] for k in ("G", "H", "G2", "H2", "E"))
    assert h.start - g.stop == bw and g.stop % bw == 0 and not (case.img[:, :17, g.stop:h.start] == fc.VAL).any()
    assert h2.start - g2.stop == 1 and not (case.img[:, :, g2.stop] == fc.VAL).any()
    assert (e.stop + 1) % bw == 0 and not (case.img[:, 16:, e.stop] == fc.VAL).any()
    a, bb, cc = (case.bodies[k][2] for k in ("A", "B", "C"))
    assert bb.stop == a.start and a.start % 64 == 0 and cc.start == a.stop and a.stop % bw == 0
    assert (a.stop % 64 != 0) == (bw < 64)
    assert case.bodies["L"][2].stop == dx
    # T: the tail's tile holds a whole block of T as well (for blocks narrower than a tile), no loose voxel lies within
    # one tile of it, and T's seed sits two tiles before it
    t = case.bodies["T"][2]
    tail_tile = (t.stop - 1) // 64
    assert t.start % 64 == 0 and (t.stop - t.start) % bw == bw // 2 and case.floods[2][1][4][0] // 64 <= tail_tile - 2
    assert ((t.stop - bw // 2) // 64 == tail_tile and (t.stop - bw // 2) % 64 == bw) == (bw < 64)
    assert not case.facts["loose"][:, :, (tail_tile - 1) * 64:(tail_tile + 2) * 64].any()


@pytest.mark.parametrize("conn", [1, 2, 3])
@pytest.mark.parametrize("dx", fc.WIDTHS)
def test_widths_cases_references_agree_and_join_what_was_built(oracle, dx, conn):
    case = fc.widths_case(dx)
    ref = fc.run_floods(case, conn, oracle.floodfill_threshold)
    lab = fc.label_floods(case, conn)
    for (name, fill, before, after), (_, _, _, after_l) in zip(ref, lab):
        assert np.array_equal(after, after_l), name
        for body, (got, cand) in fc.body_counts(case, fill, before, after).items():
            assert cand > 0 and got == (cand if body in case.joined[conn][name] else 0), (name, body, got, cand)


# ---- (c) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lanes,per_lane,on", [("rows65", 128, 1, 1), ("rows1025", 1024, 2, 1), ("rows86x85", 1024, 8, 1),
                                                    ("rows86x86", 0, 0, 0)])
def test_rows_cases_are_on_their_path(describe, name, lanes, per_lane, on):
    case = fc.rows_case(name)
    d = describe(case.shape, 1)
    assert (d[ON], d[LANES], d[ROWS_PER_LANE], d[FUSED]) == (on, lanes, per_lane, on)
    assert case.shape[2] <= 5 and case.img.size < 6.1e6
    nty, ntz, _ = fc.ROWS[name]
    assert case.facts["rows"] == nty * ntz == d[TILES]
    # the slab owns the last row of tiles (the only row of the last lane slot at 1025 rows) and every slice
    assert (case.img[:, (nty - 1) * 16:, :] == fc.VAL).all() and (case.img[:, 32:, :] == fc.VAL).all()
    assert not (case.img[:, 23:25, :] == fc.VAL).any()
    whole, exist = fc.whole_block_share(case, 1)
    assert exist == nty * ntz and whole == (nty - 1) * ntz - 2     # all but the wall's row and the two punched tiles
    if name in ("rows86x85", "rows86x86"):
        assert case.facts["hops26"] >= fc.ESCAPE


@pytest.mark.parametrize("conn", [1, 3])
@pytest.mark.parametrize("name", list(fc.ROWS))
def test_rows_cases_references_agree(oracle, name, conn):
    case = fc.rows_case(name)
    ref = fc.run_floods(case, conn, oracle.floodfill_threshold)
    lab = fc.label_floods(case, conn)
    for (fname, fill, before, after), (_, _, _, after_l) in zip(ref, lab):
        assert np.array_equal(after, after_l), fname
        for body, (got, cand) in fc.body_counts(case, fill, before, after).items():
            assert cand > 0 and got == (cand if body in case.joined[conn][fname] else 0), (fname, body, got, cand)
    assert (ref[0][3] == 1).sum() > (case.img[:, 32:, :] == fc.VAL).sum() - 16  # ... plus the wall's loose voxels it touches


# ---- (d) --------------------------------------------------------------------------------------------------------------------
def test_tile_serpentine_is_longer_than_the_escape(describe, oracle):
    case = fc.tile_serpentine()
    assert case.shape == (1, 944, 1100) and describe(case.shape, 1)[:6] == [1, 32, 2, 64, 1, 1]
    hops, all_reached = fc.tile_hops(case)
    assert all_reached and hops == case.facts["hops"] == 30 * 17 + 29 * 2 and hops > fc.ESCAPE
    (_, fill, _, after), = fc.run_floods(case, 1, oracle.floodfill_threshold)
    (_, _, _, after_l), = fc.label_floods(case, 1)
    assert np.array_equal(after, after_l) and np.array_equal(after == 1, case.img == fc.VAL)


@pytest.mark.parametrize("dx,block", zip(fc.ALL_CANDIDATE_WIDTHS, (16, 32, 64)))
def test_all_candidate_volumes(describe, oracle, dx, block):
    case = fc.all_candidate(dx)
    assert describe(case.shape, 1)[:3] == [1, block, 64 // block]
    whole, exist = fc.whole_block_share(case, 1)
    assert whole == exist
    (_, _, _, after), = fc.run_floods(case, 3, oracle.floodfill_threshold)
    assert (after == 1).all()


# ---- (e) --------------------------------------------------------------------------------------------------------------------
def test_long_list_case(describe, oracle):
    case = fc.long_list()
    (_, seeds, _), = case.floods
    d = describe(case.shape, len(seeds))
    assert (d[ON], d[BLOCK], d[FUSED], d[GRID_CAP], d[TILES]) == (1, 64, 0, 1536, 2600)
    assert len(seeds) == 5000 > fc.SEED_CHUNK and all(case.img[z, y, x] == fc.VAL for x, y, z in seeds)
    assert fc.woken_tiles(case) > fc.GRID_CAP              # the first round's list is longer than its grid
    assert fc.whole_block_share(case, 1)[0] == 0
    assert 0.61 < (case.img == fc.VAL).mean() < 0.63
    for conn in (1, 3):
        (_, _, _, after), = fc.run_floods(case, conn, oracle.floodfill_threshold)
        (_, _, _, after_l), = fc.label_floods(case, conn)
        assert np.array_equal(after, after_l) and (after == 1).mean() > 0.5


def test_ring_corridor_case(describe, oracle):
    case = fc.ring_corridor()
    d = describe(case.shape, 1)
    assert fc.RING < case.facts["tiles"] == d[TILES] == 31 < fc.ESCAPE
    assert fc.whole_block_share(case, 1)[0] == 0           # nothing for the coarse pass: the rounds walk the line
    for conn in (1, 3):
        (_, _, _, after), = fc.run_floods(case, conn, oracle.floodfill_threshold)
        (_, _, _, after_l), = fc.label_floods(case, conn)
        assert np.array_equal(after, after_l) and (after[1, 1] == 1).all()
        assert bool(after[0].any()) == (conn == 3)
