"""Every case of _ray_cases.py stands where its name says, proven without a device: the ray lengths hand over between the two
loops of k_rays_strided in every shape the loops allow, the rows fill the chunks, words and tails of k_rays_rows they claim, the
built rays break at the samples they were built for, each contour case takes the FAST variant, route and segment split it names,
the forced-open pixels are open under the restated decide rule with exactly the segment bits claimed -- and the oracle's picture
of those pixels changes when the exact pass is robbed of a segment, is given bit 0 only, or is replaced by the truncated lower
bound.  That last part is what lets test_gpu_ray_edges.py fail."""
import functools

import numpy as np
import pytest

import _ray_cases as C
import _slab_cases as sc


def _pic(oracle, vol, n, axis):
    out = np.zeros(tuple(d for i, d in enumerate(vol.shape) if i != axis), vol.dtype)
    oracle.fast_countour_mip(vol, n, axis, 0, 0, 0, out)
    return out


# ---- the strided walk ------------------------------------------------------------------------------------------------------------
def test_strided_lengths_hand_over_in_every_shape():
    """(unguarded iterations, guarded blocks): 32 is the one length at which the unguarded loop runs exactly once and leaves one
    whole block; 48 does that after two iterations; 17, 33 and 49 leave a block of one sample"""
    want = {1: (0, 1), 2: (0, 1), 15: (0, 1), 16: (0, 1), 17: (0, 2), 31: (0, 2), 32: (1, 1), 33: (1, 2), 47: (1, 2), 48: (2, 1), 49: (2, 2)}
    assert set(want) == set(C.STRIDED_LENS)
    for n, plan in want.items():
        assert C.strided_plan(n) == plan, n
    assert {C.strided_plan(n) for n in C.STRIDED_LENS} == {(u, g) for u in (0, 1, 2) for g in (1, 2)}
    # the lengths test_gpu_rays.py walks never leave one whole block behind one unguarded iteration
    assert all(C.strided_plan(n) != (1, 1) for n in (3, 7, 13, 18, 20, 24, 30, 33, 40, 45, 64, 66, 70))
    for npix in C.STRIDED_PIXELS:  # one wave short of a lane, a full wave, a wave and a lane, two blocks
        nr, nc = C.grid_of(npix)
        assert nr * nc == npix
    assert [C.cdiv(p, 64) for p in C.STRIDED_PIXELS] == [1, 1, 2, 5] and C.cdiv(257, 256) == 2


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["i16", "u8", "f64"])
def test_ray_tables_keep_rays_alive_across_every_block(dtype):
    """the drawn rays of the block-edge matrix: at every length some LMIP rays break in each 16-sample block and some never do,
    one window is entered by no sample and one holds every sample; under MIDA's narrow window some rays turn opaque in each
    block, under the wide one a quarter of the rays never does"""
    for length in C.STRIDED_LENS + C.staged_lens(dtype):
        rays = C.lmip_rays(257, length, dtype)
        assert rays.dtype == dtype and rays.shape == (1, 257, length)
        w_draw, w_all, w_none = C.LMIP_WINDOWS[dtype]
        assert ((rays >= w_all[0]) & (rays <= w_all[1])).all() and not ((rays >= w_none[0]) & (rays <= w_none[1])).any()
        if length == 1:
            continue
        _, brk = sc.lmip_walk(C.as_axis0(rays), *w_draw)
        assert (brk < 0).any()
        blocks = {int(b) // C.B for b in brk.ravel() if b >= 0}
        assert blocks >= set(range(1 if length > 17 else 0, (length - 1) // C.B + 1)), (length, blocks)
    if dtype == C.I16:
        for length in (17, 32, 33, 49, 129):
            rays = C.mida_rays(257, length, dtype)
            _, brk = sc.mida_walk(C.as_axis0(rays), *C.MIDA_WINDOWS[dtype][0])
            assert {int(b) // C.B for b in brk.ravel() if b >= 0} >= set(range((length - 1) // C.B + 1))
            _, brk = sc.mida_walk(C.as_axis0(rays), *C.MIDA_WINDOWS[dtype][1])
            assert (brk < 0).sum() >= 257 // 4


# ---- the staged walk -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=["i16", "u8", "f64"])
def test_staged_lengths_fill_the_chunks_they_claim(dtype):
    isz = dtype.itemsize
    ch = {2: 64, 1: 128, 8: 16}[isz]
    lens = C.staged_lens(dtype)
    plans = [C.staged_plan(n, isz, 0, 64) for n in lens]
    assert all(p.CH == ch and p.PER == 8 // isz for p in plans)
    assert [(p.chunks, p.last_chunk) for p in plans[:5]] == [(1, ch - 1), (1, ch), (2, 1), (2, ch), (3, 1)]
    assert [p.vec_ok for p in plans[:5]] == [False, True, False, True, False]
    odd = plans[5]
    assert (lens[5] * isz) % 16 != 0 and not odd.vec_ok and odd.chunks >= 2
    if isz < 8:  # (float64: one sample per LDS word, no tail to have)
        assert odd.tail > 0 and odd.words > 0 and plans[0].tail == 8 // isz - 1
    assert plans[6].vec_ok and (plans[6].chunks, plans[6].last_chunk) == (2, 16 // isz)
    # one element past an aligned address: the 16-byte path is off at every length
    assert not any(C.staged_plan(n, isz, isz, 64).vec_ok for n in lens)
    assert [C.staged_plan(ch, isz, 0, r).last_wave_live for r in C.STAGED_RAYS] == [1, 63, 64, 1, 63, 64, 1]
    assert [C.staged_plan(ch, isz, 0, r).waves for r in C.STAGED_RAYS] == [1, 1, 1, 2, 4, 4, 5]  # (4 waves = one workgroup)


# ---- early exit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.EXIT_CASES, ids=C.ids(C.EXIT_CASES))
def test_built_rays_break_where_they_were_built_to(oracle, case):
    vol = C.as_axis0(case.rays)
    if case.kind == "lmip":
        pic, brk = sc.lmip_walk(vol, *C.EXIT_LMIP_WINDOW)
        want = np.zeros(pic.shape, np.int16)
        oracle.lmip(vol, 0, *C.EXIT_LMIP_WINDOW, want)
    else:
        pic, brk = sc.mida_walk(vol, *C.EXIT_MIDA_WINDOW)
        want = np.zeros(pic.shape, np.int16)
        oracle.mida(vol, 0, *C.EXIT_MIDA_WINDOW, want)
    assert np.array_equal(brk, case.breaks)
    assert np.array_equal(pic, want)
    flat = brk.ravel()
    first_block = (flat[:64] >= 0) & (flat[:64] < C.B)
    if case.branch == "exit-whole-wave-in-first-block":
        assert first_block.all() and not ((flat[64:] >= 0) & (flat[64:] < C.B)).any()
        assert {int(b) for b in flat[64:]} == {16, case.length - 1, -1}
    else:
        assert first_block.sum() == 63 and flat[37] == -1
    assert {int(b) for b in flat[:64] if b >= 0} == ({1, 15} if case.kind == "lmip" else {0, 1, 15})
    # a walk that goes on past a break, or stops one sample early, ends on another value: the samples around a break differ
    if case.kind == "lmip":
        for (r, c), b in np.ndenumerate(brk):
            ray = case.rays[r, c]
            if 0 <= b < case.length - 1:
                assert ray[b + 1:].max() > want[r, c]
            if b < 0:  # (a ray that never falls answers with its last sample, which no earlier sample equals)
                assert ray[-1] == want[r, c] and ray[:-1].max() < ray[-1]


def test_exit_cases_cover_both_arrangements_and_both_walks():
    assert {(c.kind, c.branch, c.length) for c in C.EXIT_CASES} == {(k, b, n) for k in ("lmip", "mida") for n in (49, 133)
                                                                    for b in ("exit-whole-wave-in-first-block", "exit-one-lane-runs-on")}
    assert C.strided_plan(49) == (2, 2) and C.staged_plan(133, 2, 0, 128).chunks == 3
    for n in (49, 133):
        assert C.exit_depths(n) == (0, 1, 15, 16, n - 1)


# ---- min / max --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=["i16", "u8", "f64"])
def test_minmax_sizes_reach_body_tail_and_cap(dtype):
    isz = dtype.itemsize
    V = 16 // isz
    sizes = C.minmax_sizes(dtype)
    assert set(sizes) == {1, V - 1, V, V + 1, 255, 256, 257, 2048 * 256 + 5} - {0}
    plans = {n: C.minmax_plan(n, isz, 0) for n in sizes}
    assert plans[V] == (V, V, 0, 1, 0) and plans[V + 1][:3] == (V, V, 1) and plans[1][:3] == (V, 0, 1)
    if V > 2:
        assert plans[V - 1][:3] == (V, 0, V - 1)
    assert [plans[n].blocks for n in (255, 256, 257)] == [1, 1, 2]
    big = 2048 * 256 + 5
    assert C.cdiv(big, 256) == 2049 and plans[big].blocks == 2048 and plans[big].tail == big % V
    unaligned = C.minmax_plan(big, isz, isz)
    assert unaligned.body == 0 and unaligned.tail == big and unaligned.strides == 2  # five lanes go round a second time
    for n in sizes:
        spots = C.minmax_spots(n, dtype)
        p = plans[n]
        assert spots["first"] == 0 and spots["last"] == n - 1
        if p.body > 1:
            assert 0 < spots["body-middle"] < p.body and spots["body-end"] == p.body - 1
        if p.tail:
            assert p.body <= spots["tail"] < n
        base = C.minmax_base(n, dtype)
        lo, hi = C.MINMAX_ENDS[dtype]
        assert base.dtype == dtype and (base > lo).all() and (base < hi).all()
    lo, hi = C.MINMAX_ENDS[C.F64]
    assert float(np.float32(lo)) != lo and float(np.float32(hi)) != hi


# ---- the contour MaxIP: variants, routes, segments -----------------------------------------------------------------------------------
def test_every_contour_case_takes_the_branch_it_names():
    for c in C.FCM_CASES:
        plan = C.fcm_plan(c.vol.shape, c.axis, c.n, c.vol.dtype, c.offset)
        kind, _, rest = c.branch.partition("-")
        if kind == "variant":
            assert plan.route == "fused" and rest == "FAST%d-%s" % (plan.FAST, "rows" if c.axis == 2 else "walk"), c.name
            assert plan.FAST == C.VARIANT_EXPONENTS[c.n]
        elif kind == "route":
            assert rest.endswith(plan.route), c.name
            assert ("unaligned" in rest) == (c.offset % 16 != 0) and (c.offset or ("dx%d-" % c.vol.shape[2]) in rest)
        elif kind == "segments":
            length = c.vol.shape[c.axis]
            assert ("len%d-" % length) in rest and plan.route == "fused" and plan.fast
            assert (plan.split, plan.seg, plan.last_seg) == {64: (2, 32, 32), 75: (2, 38, 37), 1024: (32, 32, 32), 1030: (32, 33, 7)}[length]
            depth, s = c.depths[0], c.depths[0] // plan.seg
            where = {"first-seg": s == 0 and 0 < depth < plan.seg - 1, "last-seg": s == plan.split - 1 and depth > s * plan.seg,
                     "border-below": depth == plan.seg - 1, "border-above": depth == plan.seg,
                     "last-border-below": depth == 31 * plan.seg - 1, "last-border-above": depth == 31 * plan.seg,
                     "seg31": s == 31 and 31 * plan.seg < depth < length - 1}
            assert where[rest.split("-", 1)[1]], c.name
        else:
            assert kind == "open" and plan.route == "fused" and plan.fast and plan.FAST in (2, 3), c.name


def test_every_named_branch_has_a_case():
    have = {}
    for c in C.FCM_CASES:
        have.setdefault(c.branch, []).append(c.name)
    missing = [b for b in C.FCM_BRANCHES if b not in have]
    assert not missing, missing
    for b in C.FCM_BRANCHES:
        print("%-40s %3d cases, e.g. %s" % (b, len(have[b]), have[b][0]))
    # the variants the suite never ran before: the exact walk, the exact rows, and the combine over more than one segment
    exact = [c for c in C.VARIANT_CASES if C.fcm_plan(c.vol.shape, c.axis, c.n).FAST == 0]
    assert {c.axis for c in exact} == {0, 1, 2} and {c.n for c in exact} == {0.0, 100.0}
    assert any(C.fcm_plan(c.vol.shape, c.axis, c.n).split == 2 and C.fcm_plan(c.vol.shape, c.axis, c.n).last_seg == 37 for c in exact)
    # FAST 1 through both kernels, ragged split included
    half = [C.fcm_plan(c.vol.shape, c.axis, c.n) for c in C.VARIANT_CASES if c.n == 0.5]
    assert {p.FAST for p in half} == {1} and any(p.split == 2 for p in half)
    # the top bit of the segment word
    assert any(c.expect_bits == (31,) for c in C.SEGMENT_CASES) and np.uint32(1) << np.uint32(31) == 0x80000000
    # the other families, by name
    for name in ["strided-handover-%d+%d" % p for p in sorted({C.strided_plan(n) for n in C.STRIDED_LENS})]:
        print(name)
    for c in C.EXIT_CASES:
        print(c.branch, c.name)
    for dt in C.DTYPES:
        for off in (0, dt.itemsize):
            shapes = {"staged-%s-%s-%dchunks-last%s%s" % (dt.name, "vec" if p.vec_ok else "elementwise", p.chunks,
                                                            "full" if p.last_chunk == p.CH else "short", "-tail" if p.tail else "")
                      for p in (C.staged_plan(n, dt.itemsize, off, 64) for n in C.staged_lens(dt))}
            assert len(shapes) >= (5 if off == 0 else 4), shapes
            print("\n".join(sorted(shapes)))
        kinds = {"minmax-%s-%s%s%s" % (dt.name, "body" if p.body else "nobody", "-tail" if p.tail else "", "-capped" if p.blocks == 2048 else "")
                 for p in (C.minmax_plan(n, dt.itemsize, off) for n in C.minmax_sizes(dt) for off in (0, dt.itemsize))}
        assert {k.split("-", 2)[2] for k in kinds} >= {"body", "body-tail", "nobody-tail", "body-tail-capped", "nobody-tail-capped"}, kinds
        print("\n".join(sorted(kinds)))


@pytest.mark.parametrize("n", [0.0, 100.0])
def test_oracle_accepts_the_exponents_of_the_exact_fold(oracle, n):
    """powf(base, 0) is 1 for every base (0 included: the value is the gradient's magnitude), powf(base, 100) is tiny except
    where the ray runs across the gradient; neither leaves int16, so the reference does not panic and the GPU must not refuse"""
    for shape in C.VARIANT_SHAPES:
        vol = next(c.vol for c in C.VARIANT_CASES if c.vol.shape == shape)
        for axis in range(3):
            assert _pic(oracle, vol, n, axis).any(), (shape, axis)


def test_route_volumes_have_gradients_on_their_first_and_last_rows_and_columns(oracle):
    for c in C.ROUTE_CASES:
        pic = _pic(oracle, c.vol, c.n, c.axis)
        for edge in (pic[0], pic[-1], pic[:, 0], pic[:, -1]):
            assert edge.any(), c.name


# ---- the contour MaxIP: pixels forced open ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _classified(name):
    c = next(c for c in C.FORCED_OPEN_CASES if c.name == name)
    return C.classify(c.vol, c.n, c.axis)


@pytest.mark.parametrize("case", C.FORCED_OPEN_CASES, ids=C.ids(C.FORCED_OPEN_CASES))
def test_forced_open_pixels_are_open_and_only_the_exact_pass_can_settle_them(oracle, case):
    k = _classified(case.name)
    plan = k.plan
    pic = _pic(oracle, case.vol, case.n, case.axis)
    inner = C.interior(pic.shape)
    assert inner.sum() >= 6
    # the true maximum is the integer itself, strictly inside its bounds: open, with exactly the claimed segments
    assert (pic[inner] == case.value).all()
    assert k.open[inner].all(), "decided: %s" % np.argwhere(inner & ~k.open)[:3]
    assert (k.lo[inner] < case.value).all() and (k.hi[inner] > case.value).all()
    assert (case.value - k.lo[inner] < 1e-2).all() and (k.hi[inner] - case.value < 1e-2).all()  # (and not by much: the bounds are tight)
    bits = sum(1 << s for s in case.expect_bits)
    assert (k.mask[inner] == bits).all(), (hex(bits), [hex(int(m)) for m in np.unique(k.mask[inner])])
    holds = C.value_bits(case)
    assert tuple(sorted({d // plan.seg for d in case.depths})) == tuple(holds) and set(holds) <= set(case.expect_bits)
    # the oracle's contour volume, ray axis first
    tmp = np.moveaxis(oracle.fcm_volume(case.vol, case.n, case.axis), case.axis, 0)
    assert np.array_equal(tmp.max(0), pic)
    length = tmp.shape[0]
    seg_of = np.arange(length) // plan.seg
    # (1) an open segment's voxels left out: the one that holds the value.  Where several hold it (the equal mirror, the plain
    #     ramp) any single one is made up for by the others -- which is stated, not hidden -- and all of them together are not.
    without_all = tmp[~np.isin(seg_of, holds)].max(0) if len(holds) < plan.split else np.zeros_like(pic)
    assert (without_all[inner] < pic[inner]).all()
    if plan.split > len(holds):  # what is left are decoys, lower by less than one
        assert (without_all[inner] == case.value - 1).all()
    if len(holds) > 1:
        for s in holds:
            assert np.array_equal(tmp[seg_of != s].max(0)[inner], pic[inner])
    # (2) only bit 0 of the mask honoured: wrong exactly where the maximum lies in a later segment
    bit0 = np.where(k.open, tmp[seg_of == 0].max(0), pic)
    assert (bit0[inner] != pic[inner]).all() == (0 not in holds), case.name
    if 0 in holds:
        assert np.array_equal(bit0[inner], pic[inner])
    # (3) the value rounded the wrong way by one: the truncated lower bound, what deciding the pixel would have written
    assert (np.trunc(k.lo[inner]).astype(np.int64) == case.value - 1).all()
    assert (np.trunc(k.hi[inner]).astype(np.int64) == pic[inner]).all()
    # and the pixels around the interior are not all open: both outcomes of the decide rule occur in the case
    assert (~k.open).any() or case.branch == "open-every-interior-pixel"


def test_forced_open_cases_make_each_recomputation_tell():
    """(1) tells on every case with one open segment in a split ray, (2) on every case whose maximum is behind segment 0 -- both
    axes that split, both exponents, the top segment included; (3) tells on every case"""
    single = [c for c in C.FORCED_OPEN_CASES if len(C.value_bits(c)) == 1 and C.fcm_plan(c.vol.shape, c.axis, c.n).split > 1]
    later = [c for c in C.FORCED_OPEN_CASES if 0 not in C.value_bits(c)]
    # the decoy that stays open although it is one lower: both bits set, the value in one segment only -- in either
    lower = [c for c in C.OPEN_CASES if c.branch == "open-mirror-lower-decoy"]
    assert {(c.axis, c.n, C.value_bits(c)) for c in lower} == {(a, n, b) for a in (0, 1) for n in (1.0, 2.0) for b in ((0,), (1,))}
    assert all(c.expect_bits == (0, 1) for c in lower)
    for group in (single, later):
        assert {(c.axis, c.n) for c in group} == {(a, n) for a in (0, 1) for n in (1.0, 2.0)}
    assert any(c.expect_bits == (31,) for c in later) and any(c.expect_bits == (1,) for c in later)
    mirrors = [c for c in C.OPEN_CASES if c.branch == "open-mirror-two-bits"]
    assert {c.expect_bits for c in mirrors if c.axis != 2} == {(0, 1)} and {c.expect_bits for c in mirrors if c.axis == 2} == {(0,)}
    assert {c.axis for c in C.OPEN_CASES} == {0, 1, 2} and {c.n for c in C.OPEN_CASES} == {1.0, 2.0}


def test_decoys_are_lower_by_less_than_one_and_by_more_than_the_bound(oracle):
    """at a depth next to the feature the contour value is c - 0.5 (exponent 1) or c - 0.9 .. c - 0.95 (exponent 2): the oracle's
    truncated contour volume holds c - 1 there, and the restated bounds of the pixel are five orders of magnitude narrower"""
    for case in C.OPEN_CASES:
        if case.branch != "open-feature-and-decoys":
            continue
        tmp = np.moveaxis(oracle.fcm_volume(case.vol, case.n, case.axis), case.axis, 0)
        inner = C.interior(tmp.shape[1:])
        depth = case.depths[0]
        for d in (depth - 1, depth + 1):
            assert (tmp[d][inner] == case.value - 1).all(), case.name
        assert (tmp[depth][inner] == case.value).all()
        k = _classified(case.name)
        assert ((k.hi - k.lo)[inner] < 1e-4).all()


def test_every_volume_is_small():
    for c in C.FCM_CASES:
        assert c.vol.size <= 40000 and c.vol.dtype == np.int16, c.name
    for c in C.EXIT_CASES:
        assert c.rays.size <= 20000
    assert max(C.STRIDED_LENS) * max(C.STRIDED_PIXELS) <= 20000
    for dt in C.DTYPES:
        assert max(C.staged_lens(dt)) * max(C.STAGED_RAYS) * dt.itemsize <= 400000
