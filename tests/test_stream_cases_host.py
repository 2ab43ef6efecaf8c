"""The case tables of _stream_cases.py, checked without a GPU: every named case takes the branch its id names (from the launch
arithmetic of the .hip files restated there), and every new reference agrees with an independent statement of the same thing.
The GPU half is test_gpu_stream_edges.py."""
import math
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage

import _stream_cases as C


# ---- projections ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,shape,want", C.MIP_SPLIT_CASES, ids=[c[0] for c in C.MIP_SPLIT_CASES])
def test_mip_split_plan_table(cid, shape, want):
    for axis in (0, 1):
        slab = shape if axis == 0 else (shape[1], shape[0], shape[2])
        plan = C.mip_plan_of(slab, axis)
        for k, v in want.items():
            assert plan[k] == v, (cid, axis, k, plan)
        assert (plan["split"] - 1) * plan["seg"] < shape[0] <= plan["split"] * plan["seg"] and 1 <= plan["last"] <= plan["seg"]
        assert plan["seg"] <= C.MIP_MAX_SEG  # int32 partial sums: 32767 * 65535 < 2^31
        if plan["split"] > 1:
            assert plan["seg"] >= C.MIP_MIN_SEG


def test_mip_split_shrinks_only_where_named():
    shrunk = [cid for cid, shape, _ in C.MIP_SPLIT_CASES if C.mip_plan_of(shape, 0)["first"] != C.mip_plan_of(shape, 0)["split"]]
    assert shrunk == ["mip-split-2048to2000"]
    assert 32767 * 65535 < 2 ** 31


def test_mip_row_and_u8_cases_hit_both_sides():
    seen = set()
    for length in C.MIP_ROW_LENGTHS:
        seen |= {C.mip_rows_branch(r, length) for r in range(5)}
    assert seen == {"scalar", "vec", "vec+tail", "vec0+tail"}
    assert {C.mip_rows_branch(r, 512, base_offset=2) for r in range(5)} == {"scalar"}  # the volume at vol.at(2)
    assert C.mip_rows_branch(0, 1) == "vec0+tail" and C.mip_rows_branch(1, 7) == "scalar" and C.mip_rows_branch(3, 8) == "vec"
    # uint8: a lane owns 16 pixels; 15 -> one partial group, 16 -> one full, 17 / 33 -> full groups and a partial one
    assert [(C.cdiv(w, 16), w % 16) for w in C.MIP_U8_WIDTHS] == [(1, 15), (1, 0), (2, 1), (3, 1)]


def test_replicate_cases_take_their_branches():
    b = {c: C.replicate_branch(*c) for c in C.REPLICATE_CASES}
    assert [c for c in C.REPLICATE_CASES if b[c]["fast"]] == [(5, 8, 1), (3, 4, 2), (16, 16, 4), (2, 6, 4)]
    assert [c for c in C.REPLICATE_CASES if b[c]["straddles"]] == [(3, 5, 1), (7, 3, 3), (3, 3, 1), (1, 1, 7), (9, 5, 3)]
    assert b[(1, 1, 1)] == dict(fast=False, straddles=False, partial=True) and b[(1, 1, 7)]["partial"] and b[(9, 5, 3)]["partial"]
    assert len({C.replicate_id(*c) for c in C.REPLICATE_CASES}) == len(C.REPLICATE_CASES)
    src = C.replicate_src(3, 5)
    want = C.replicate_ref(src, 3)
    assert want.shape == (9, 15) and all(want[y, x] == src[y // 3, x // 3] for y in range(9) for x in range(15))
    assert src.min() == C.I16_MIN and src.max() == C.I16_MAX


# ---- the vec switches ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(C.VEC_KERNELS))
def test_vec_cases_cover_every_branch(kernel):
    cases = C.vec_cases(kernel)
    ptrs, min_n, chunk = C.VEC_KERNELS[kernel]
    assert len({cid for cid, _, _ in cases}) == len(cases) == len(C.VEC_N) * (1 + sum(len(o) for _, _, o in ptrs))
    by = {(n, tuple(offs.items())): cid.split("-")[1] for cid, n, offs in cases}
    for n in C.VEC_N:
        want = "scalar" if n < min_n else ("vec+tail" if n % chunk else "vec")
        assert by[(n, ())] == want
        for name, _, offs in ptrs:
            for o in offs:
                assert by[(n, ((name, o),))] == "scalar"  # one offset pointer is enough to leave the vector body
    assert {b for b in by.values()} == {"scalar", "vec", "vec+tail"}
    # offsets never misalign an element of its own type
    for name, _, offs in ptrs:
        assert all(o % (2 if name in ("img", "out") and kernel in ("lut", "density") else 1) == 0 for o in offs)


def test_density_mask_offset_4_defeats_only_the_8_byte_test():
    assert C.vec_branch("density", 16, {"mask": 4}) == "scalar" and C.vec_branch("density", 16, {"mask": 8}) == "vec"
    assert C.vec_branch("density", 16, {"img": 8}) == "scalar" and C.vec_branch("density", 16, {"img": 16}) == "vec"


def test_density_and_std_references_agree_with_numpy():
    rng = np.random.default_rng(1)
    img = rng.integers(-32768, 32768, (6, 7, 9)).astype(np.int16)
    sel = rng.random(img.shape) < 0.5
    cnt, s1, s2, lo, hi = C.density_ref(img, sel)
    v = img[sel].astype(np.int64)
    assert (cnt, s1, s2, lo, hi) == (v.size, int(v.sum()), int((v * v).sum()), int(v.min()), int(v.max()))
    assert C.density_ref(img, np.zeros(img.shape, bool)) == (0, 0, 0, 32767, -32768)
    assert C.exact_std(v) == pytest.approx(float(v.std()), rel=1e-13)
    assert C.float_formula_std(v) == pytest.approx(float(v.std()), rel=1e-10)  # noisy data does not cancel: why nobody noticed


@pytest.mark.parametrize("cid,base,odd", C.STD_CASES, ids=[c[0] for c in C.STD_CASES])
def test_std_cases_and_the_old_formula(cid, base, odd):
    """the new check has teeth: sqrt(E[x^2] - mean^2) in float64 misses rel=1e-10 on the two nearly constant selections"""
    img, m = C.std_case(base, odd)
    vals = img[m[1:, 1:, 1:] > 127]
    assert vals.size == 100001 and int((vals == base).sum()) == (100001 if odd == base else 100000)
    want = float(vals.std())
    assert C.exact_std(vals) == pytest.approx(want, rel=1e-10)
    old = C.float_formula_std(vals)
    if odd == base:
        assert want == 0.0 and C.exact_std(vals) == 0.0
    else:
        assert abs(old - want) > 1e-10 * want, (old, want)
        assert abs(old - want) / want > 1e-6
    # the exact value itself, from the definition: one voxel differs by 1 -> variance (n - 1) / n^2
    if odd != base:
        n = 100001
        assert C.exact_std(vals) == math.sqrt(float(Fraction(n - 1, n * n)))


def test_lut_windows_stay_in_the_references_domain():
    a = C.all_int16()
    assert a.size == 65536 and np.array_equal(np.sort(a.ravel()), np.arange(-32768, 32768))
    assert all(ww <= 32767 for ww, _ in C.LUT_WINDOWS)
    b = a.copy()
    b[b == -32768] = 0
    assert np.array_equal(C.min_shift_ref(a).astype(np.int64), a.astype(np.int64) + 32768) and C.min_shift_ref(a).max() == 65535
    assert np.array_equal(C.min_shift_ref(b).astype(np.int64), b.astype(np.int64) + 32767)


# ---- mask edits and counts -------------------------------------------------------------------------------------------------
def test_count_cases_take_their_paths():
    ids = [c[0] for c in C.COUNT_CASES]
    assert len(set(ids)) == len(ids)
    assert C.count_branch(4095) == "lds" and C.count_branch(4096) == "global"
    for cid, n, nreg, dt in C.COUNT_CASES:
        assert cid.split("-")[1] == C.count_branch(nreg)
        lab = C.count_labels(n, nreg, dt)
        assert lab.dtype == dt and lab.shape == (1, 1, n) and lab.min() >= 0 and lab.max() <= nreg
        if n > nreg:
            assert np.bincount(lab.ravel().astype(np.int64), minlength=nreg + 1).min() >= 1  # every bin, the last LDS one included
    assert ("count-lds-4095-int16" in ids) and ("count-global-4096-int16" in ids) and ("count-global-70000-int32" in ids)
    assert "count-global-70000-int16" not in ids
    # the loop of the histogram kernel: four trips per lane below the grid cap, more above it
    assert C.count_hist_launch(1100000) == (1075, 4) and C.count_hist_launch(2200000) == (2048, 5)
    assert C.count_hist_launch(257) == (1, 2) and C.count_hist_launch(1) == (1, 1)


@pytest.mark.parametrize("shape", C.CUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cut_camera_puts_voxels_on_both_sides(shape):
    m, mv, depth = C.cut_camera(shape)
    g = C.cut_geometry(shape, C.CUT_SPACING, m, mv)
    assert (g["q3"] <= 0).any() and (g["q3"] > 0).any()  # part of the volume is behind the eye
    front = g["q3"] > 0
    assert (g["dist"][front] <= depth).any() and (g["dist"] > depth).any()  # the depth limit cuts through
    assert (C.cut_mask(shape) > 127).sum() > 0.5 * g["q3"].size


def test_cut_cases_wrap_rows_and_slices_inside_a_chunk():
    assert [C.cut_branch(s) for s in C.CUT_SHAPES] == ["vec+tail", "vec+tail", "vec", "vec", "scalar"]
    assert C.CUT_SHAPES[0][2] == 1 and C.CUT_SHAPES[1][1] == 1  # width 1: x wraps every voxel; height 1: y wraps every row
    d, h, w = C.CUT_SHAPES[0]
    assert 16 > h * w  # one 16-voxel chunk crosses a slice
    # some voxel in front of the eye of the widest case projects off the 6 x 7 screen: the edit-mode branch decides
    m, mv, depth = C.cut_camera((3, 5, 16))
    g = C.cut_geometry((3, 5, 16), C.CUT_SPACING, m, mv)
    front = (g["q3"] > 0) & (g["dist"] <= depth)
    px, py = (g["sx"] / 2 + 0.5) * 6, (g["sy"] / 2 + 0.5) * 5
    off = front & ~((px >= 0) & (px < 7) & (py >= 0) & (py < 6))
    assert off.any() and (front & ~off).any()
    assert C.cut_screen("1x1").shape == (1, 1) and C.cut_screen("6x7").shape == (6, 7)


def test_brush_cases():
    by = {c[0]: c[1:] for c in C.BRUSH_CASES}
    shape, sp, ce, r = by["brush-on-voxel-integer-radius"]
    d2 = C.brush_dist_sq(shape, sp, ce)
    assert (d2 == r * r).sum() >= 6 and (d2 < r * r).any() and (d2 > r * r).any()  # voxels exactly on the sphere: `<=` includes them
    shape, sp, ce, r = by["brush-centre-past-far-faces-clipped-box"]
    assert all(c > s - 1 for c, s in zip(ce, shape[::-1])) and (C.brush_dist_sq(shape, sp, ce) <= r * r).any()
    shape, sp, ce, r = by["brush-centre-past-far-faces-empty-box"]
    assert math.floor((ce[0] - r) / sp[0]) > shape[2] - 1 and not (C.brush_dist_sq(shape, sp, ce) <= r * r).any()
    shape, sp, ce, r = by["brush-anisotropic"]
    inside = C.brush_dist_sq(shape, sp, ce) <= r * r
    assert len(set(sp)) == 3 and inside.any() and not inside.all()


# ---- area, holes, jump flooding -----------------------------------------------------------------------------------------------
def test_area_shapes_and_exact_spacings():
    n = {cid: s[0] * s[1] * s[2] for cid, s in C.AREA_SHAPES}
    assert n["area-2047-one-block"] == 2047 and n["area-2048-one-full-block"] == 2048 and n["area-2049-two-blocks"] == 2049
    assert n["area-one-block-210"] < C.AREA_VOXELS_PER_BLOCK
    assert [s.index(1) for cid, s in C.AREA_SHAPES if cid.startswith("area-extent1")] == [0, 1, 2]
    for sx, sy, sz in C.AREA_EXACT_SPACINGS:
        for t in (sx * sy, sx * sz, sy * sz, 2 * sx * sy + 2 * sx * sz + 2 * sy * sz):
            assert (t * 8).is_integer()  # every term a multiple of 1/8, totals far below 2^53: exact in any order
    sx, sy, sz = C.AREA_INEXACT_SPACING
    assert not (sx * sy * 2 ** 20).is_integer()
    assert 65 * 256 * 256 > C.CONVOLVE_GRID_CAP * 256  # the convolve_non_zero grid makes a second trip


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_holes_cases_are_what_they_say(kind):
    m, max_size = C.holes_case(kind)
    inner = m[1:, 1:, 1:]
    assert inner.shape == C.HOLES_SHAPE and C.cdiv(inner.shape[2], 64) == 2
    selected = int((inner > 127).sum())
    lab, nlab = ndimage.label(~(inner > 127), ndimage.generate_binary_structure(3, 1))
    sizes = np.bincount(lab.ravel())[1:]
    small = int((sizes <= max_size).sum())
    if kind == "a":
        assert selected == max_size == 5 and nlab == 1 and small == 0  # label 0 alone is small
    elif kind == "b":
        assert selected == max_size == 11 and nlab == 2 and sorted(sizes)[0] == 1 and small == 1
    else:
        assert max_size == selected - 1 and small == 0  # nothing is small: the call returns False
    assert (inner[:, :, 64:] > 127).any() and (inner[:, :, :64] > 127).any()  # both words of a row


def test_label_volume_layout():
    for nlabels in (255, 256, 257):
        lab = C.label_volume(nlabels).ravel()
        assert len(set(lab[:64])) == 1 and len(set(lab[64:128])) == 64 and lab.max() == nlabels
        assert C.cdiv(nlabels + 1, 256) == (1 if nlabels == 255 else 2)  # the block edge of k_any_small


def test_jump_cases():
    by = {c[0]: c[1:] for c in C.JUMP_CASES}
    assert by["jump-normalise-lds-1024"][1] == C.JF_LDS_SITES and by["jump-normalise-global-1025"][1] == C.JF_LDS_SITES + 1
    assert [C.jump_steps(s) for s in ((1, 1, 1), (1, 1, 2), (2, 3, 1), (8, 16, 32))] == [0, 1, 1, 5]
    s = C.jump_sites((8, 16, 32), 1025)
    assert s.shape == (1025, 3) and len({tuple(r) for r in s}) == 1025 and (s < (8, 16, 32)).all() and s.min() >= 0


# ---- synthetic volume ------------------------------------------------------------------------------------------------------------
def test_synth_hash_matches_python_ints():
    g = np.array([0, 1, 2159, 2 ** 32 - 1, 2 ** 32, 2 ** 33 + 12345, 2048 ** 3 - 2], np.uint64)
    h1, h2 = C.synth_hash(g, C.SYNTH_SEED)
    for i, gi in enumerate(g.tolist()):
        assert (int(h1[i]), int(h2[i])) == C.synth_hash_py(gi, C.SYNTH_SEED)
    assert len(set(h1.tolist())) == len(g) - 1  # the low word alone feeds h1: 0 and 2^32 share it, h2 tells them apart
    assert int(h2[0]) != int(h2[4])


def test_synth_reference_is_slab_invariant_and_bounded():
    blobs = C.synth_blobs()
    whole = C.synth_field((12, 9, 20), 0, 12, C.SYNTH_SEED, blobs)
    for z0, dz in ((0, 5), (5, 6), (11, 1)):
        assert np.array_equal(C.synth_field((dz, 9, 20), z0, 12, C.SYNTH_SEED, blobs), whole[z0:z0 + dz])
    assert not np.array_equal(C.synth_field((12, 9, 20), 0, 12, C.SYNTH_SEED + 1, blobs), whole)
    assert np.isfinite(whole).all()


@pytest.mark.parametrize("cid,shape", C.SYNTH_CASES, ids=[c[0] for c in C.SYNTH_CASES])
def test_synth_float32_spread_is_below_one_hu(cid, shape):
    """measured here: the spread is a few 1e-4 HU (float32 rounding of values up to ~2000), so the tolerance is 2 HU"""
    assert C.synth_tolerance(shape) == 2
