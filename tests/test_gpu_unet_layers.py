"""The U-Net's kernels one layer at a time (k_unet.hip: k_conv<MT, NT, KIND>, k_pool, k_head, and the weight packing the
loader shares with the diagnostic entry points), against the float64 layers of tests/_unet_ref.py.

The convolutions are checked for equality, not within a tolerance: activations in {0..7}, weights in {-3..3} \\ {0} and
integer biases make every partial sum an integer below 2^24, so float32 is exact in any summation order and one wrong,
missing or doubled product fails at any K.  Each case first asserts that precondition on conv(|x|, |w|) + |b|.

Which test launches which instantiation (KIND 0 = conv 5^3, 1 = transposed conv): every tile shape the entry point
accepts for the case's cout, forced one after the other, then run_conv's own choice (1 x 1 at these sizes):

    test_conv_exact[1->8 S5 nb3], [16+16->16 S3 nb5]                 (1,1) (2,1) (4,1) (8,1)                    KIND 0
    test_conv_exact[32->32 S2 nb7]                                   (1,1) (2,1) (4,1) (2,2) (4,2)              KIND 0
    test_conv_exact[64->128 S1 nb9], [64->128 S3 nb2],
                   [128->64 S3 nb1], [64+64->64 S2 nb3]              (1,1) (2,1) (4,1) (2,2) (4,2) (4,4)        KIND 0
    test_upconv_exact[128->64 *]                                     (1,1) (2,1) (4,1) (2,2) (4,2) (4,4)        KIND 1
    test_upconv_exact[64->32 *]                                      (1,1) (2,1) (4,1) (2,2) (4,2)              KIND 1
    test_upconv_exact[32->16 *], [16->8 *]                           (1,1) (2,1) (4,1) (8,1)                    KIND 1
    test_tile_shapes_give_the_same_bits[*]                           the same sets, on real-valued data         KIND 0, 1

(4, 4) runs only because it is forced: run_conv takes it from 607 patches of 48^3 in one batch, which no test can afford.
test_gpu_segment.py reaches (2, 2) and (4, 2) through the public forward as well.

The transposed conv always launches 8 x tiles x column groups waves, a multiple of four, so every block is full and its
`cls >= 8` exit cannot be reached by any launch; the conv's `m0 >= nvox` exit runs wherever the wave count is not a
multiple of four (375 voxels at MT = 4: 6 waves, MT = 8: 3 waves).
"""
import ctypes
import functools

import numpy as np
import pytest

import _unet_ref as R

gpu = pytest.mark.gpu


def real_case(kind, c0, c1, cout, S, nb, seed):
    rng = np.random.default_rng(seed)
    cin = c0 + c1
    x = rng.standard_normal((nb, S, S, S, cin)).astype(np.float32)
    wshape = (cout, cin, 5, 5, 5) if kind == 0 else (cin, cout, 4, 4, 4)
    return x, rng.standard_normal(wshape).astype(np.float32), rng.standard_normal(cout).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_data(kind, c0, c1, cout, S, nb, real=False):
    """(x, w, b, float64 result, float64 result of the absolute values) of one case, computed once"""
    seed = [kind, c0, c1, cout, S, nb, int(real)]
    x, w, b = (real_case if real else R.int_case)(kind, c0, c1, cout, S, nb, seed)
    want = R.ref_layer(kind, x, w, b)
    mag = R.ref_layer(kind, np.abs(x), np.abs(w), np.abs(b))
    for a in (x, w, b, want, mag):
        a.setflags(write=False)
    return x, w, b, want, mag


def run_case(kind, c0, c1, x, w, b, tile, relu=False):
    from invesalius3_amd import segment as sg
    return sg.conv_layer(kind, x[..., :c0], w, b, x[..., c0:] if c1 else None, relu=relu, tile=tile)


#            cin (two numbers: the two sources of a torch.cat), cout, S, nb
CONV_CASES = [
    (1, 0, 8, 5, 3),     # 375 voxels: a row tail for every MT; cin padded to 4; partial column tile; all 125 taps in bounds
    (16, 16, 16, 3, 5),  # 135 voxels; concat order; every tap in bounds for some voxel; leakage across patches
    (32, 0, 32, 2, 7),   # 56 voxels; NT = 2
    (64, 0, 128, 1, 9),  # only the centre tap; eight column tiles
    (64, 0, 128, 3, 2),  # 54 voxels
    (128, 0, 64, 3, 1),  # 27 voxels; (4, 4) with a single partly filled row tile
    (64, 64, 64, 2, 3),  # the deep decoder's concat
]
UP_PAIRS = [(128, 64), (64, 32), (32, 16), (16, 8)]
UP_CASES = [(cin, 0, cout, S, nb) for cin, cout in UP_PAIRS for S in (1, 2, 3) for nb in (1, 5)]
REAL_CASES = [(0,) + CONV_CASES[1], (0,) + CONV_CASES[2], (0,) + CONV_CASES[5], (1, 128, 0, 64, 2, 5), (1, 16, 0, 8, 3, 5)]


def _id(c):
    c = c[-5:]
    return "%s->%d S%d nb%d" % ("%d+%d" % c[:2] if c[1] else "%d" % c[0], c[2], c[3], c[4])


# -- on the CPU: the preconditions of the exact comparison, the rule's replay ---------------------------------------
@pytest.mark.parametrize("case", [(0,) + c for c in CONV_CASES] + [(1,) + c for c in UP_CASES], ids=_id)
def test_integer_cases_are_exact_in_float32(case):
    x, w, b, want, mag = case_data(*case)
    assert mag.max() < 2 ** 24  # every partial sum is an integer float32 holds
    assert all(np.array_equal(a, np.round(a)) for a in (x, w, b))
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    assert (x.size < 1000 or 0.2 < (x == 0).mean() < 0.3) and not (w == 0).any()
    assert (want > 0).any() and (want < 0).any()


def test_allowed_tiles_and_the_rule_agree():
    assert R.allowed_tiles(8) == R.allowed_tiles(16) == [(1, 1), (2, 1), (4, 1), (8, 1)]
    assert R.allowed_tiles(32) == R.allowed_tiles(48) == [(1, 1), (2, 1), (4, 1), (2, 2), (4, 2)]
    assert R.allowed_tiles(64) == R.allowed_tiles(128) == [(1, 1), (2, 1), (4, 1), (2, 2), (4, 2), (4, 4)]
    # whatever the rule picks is allowed, at any size
    for kind in (0, 1):
        for cout in (8, 16, 32, 48, 64, 128):
            for nvox in (1, 100, 4096, 2 ** 15, 2 ** 16, 2 ** 17, 2 ** 20, 2 ** 24):
                assert R.pick_tile(kind, nvox, cout) in R.allowed_tiles(cout)
    # the network's layers at 48^3: (4, 4) from 607 patches on, for the 64-channel layers at S = 6
    assert R.pick_tile(0, 606 * 216, 64) != (4, 4) and R.pick_tile(0, 607 * 216, 64) == (4, 4)
    assert R.pick_tile(0, 1024 * 64, 32) == (2, 2) and R.pick_tile(0, 2048 * 64, 32) == (4, 2)
    assert R.pick_tile(1, 1024 * 8, 32) == (2, 2) and R.pick_tile(1, 2048 * 8, 32) == (4, 2)


REFUSED = [  # (kind, c0, c1, cout, (mt, nt))
    (0, 8, 0, 64, (3, 1)), (0, 8, 0, 64, (1, 2)), (0, 8, 0, 64, (8, 2)), (0, 8, 0, 64, (4, 3)), (0, 8, 0, 64, (2, 4)),
    (0, 8, 0, 64, (0, 1)), (0, 8, 0, 64, (1, 0)), (0, 8, 0, 64, (-1, 1)), (1, 8, 0, 64, (16, 1)),  # not instantiated
    (0, 8, 0, 16, (2, 2)), (0, 8, 0, 16, (4, 2)), (1, 8, 0, 8, (2, 2)),                             # NT = 2 needs cout > 16
    (0, 8, 0, 16, (4, 4)), (0, 8, 0, 48, (4, 4)), (1, 8, 0, 32, (4, 4)),                            # (4, 4) needs cout > 48
    (0, 8, 0, 17, (8, 1)), (0, 8, 0, 32, (8, 1)), (1, 8, 0, 64, (8, 1)),                            # (8, 1) needs cout <= 16
    (0, 6, 6, 8, (0, 0)), (0, 1, 3, 8, (1, 1)), (1, 2, 2, 8, (0, 0)),                               # the step would straddle
]


def _refusals(on_device):
    """every refused call returns IVX_EINVAL and leaves dst as it was.  The refusal comes before the first device call,
    so without a device host arrays stand in for the activations."""
    from invesalius3_amd import _lib
    from invesalius3_amd.device import DeviceBuffer

    lib = _lib.lib()
    S, nb = 2, 2
    for kind, c0, c1, cout, (mt, nt) in REFUSED:
        cin = c0 + c1
        w = np.ones(cout * cin * (125 if kind == 0 else 64), np.float32)
        b = np.ones(cout, np.float32)
        x0, x1 = np.ones(nb * S ** 3 * c0, np.float32), np.ones(nb * S ** 3 * max(c1, 1), np.float32)
        dst = np.full(nb * (S * (1 + kind)) ** 3 * cout, 7.0, np.float32)
        used = (ctypes.c_int(-5), ctypes.c_int(-5))
        if on_device:
            bufs = [DeviceBuffer(a.nbytes) for a in (x0, x1, dst)]
            for buf, a in zip(bufs, (x0, x1, dst)):
                buf.upload(a)
            p0, p1, pd = (buf.ptr for buf in bufs)
        else:
            p0, p1, pd = _lib.ptr(x0), _lib.ptr(x1), _lib.ptr(dst)
        rc = lib.ivx_dev_unet3d_conv_layer(kind, p0, c0, p1 if c1 else None, c1, _lib.ptr(w), _lib.ptr(b), cout, S, nb, 0, mt, nt,
                                           pd, ctypes.byref(used[0]), ctypes.byref(used[1]), None)
        what = (kind, c0, c1, cout, mt, nt)
        assert rc == _lib.IVX_EINVAL, what
        assert (used[0].value, used[1].value) == (-5, -5), what
        if on_device:
            _lib.synchronize()
            assert (bufs[2].download(dst.shape, np.float32) == 7.0).all(), what
            for buf in bufs:
                buf.close()


def test_refusals_come_before_any_device_call():
    from invesalius3_amd import _lib
    _refusals(on_device=_lib.device_count() > 0)


# -- on the GPU ------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_launch_nothing(ivxlib):
    from invesalius3_amd import segment as sg
    _refusals(on_device=True)
    x, w, b = R.int_case(0, 8, 0, 16, 2, 2, 1)
    with pytest.raises(TypeError):
        sg.conv_layer(0, x, w, b, tile=(2, 2))
    with pytest.raises(TypeError):
        sg.conv_layer(0, x[..., :6], w[:, :7], b, x[..., 6:7])


def _exact(ivxlib, case):
    kind, c0, c1, cout = case[:4]
    x, w, b, want, mag = case_data(*case)
    assert mag.max() < 2 ** 24
    want32 = want.astype(np.float32)
    nvox = x.shape[0] * x.shape[1] ** 3
    for tile in R.allowed_tiles(cout) + [(0, 0)]:
        got, used = run_case(kind, c0, c1, x, w, b, tile)
        assert used == (tile if tile != (0, 0) else R.pick_tile(kind, nvox, cout)), (tile, used)
        bad = np.argwhere(got != want32)
        assert got.shape == want32.shape and not len(bad), "tile %s: %d of %d wrong, first at (n, z, y, x, c) = %s" % (
            tile, len(bad), got.size, bad[:1].tolist())
    return x, w, b, want32


@gpu
@pytest.mark.parametrize("case", CONV_CASES, ids=_id)
def test_conv_exact(ivxlib, case):
    c0, c1 = case[:2]
    x, w, b, want32 = _exact(ivxlib, (0,) + case)
    got, _ = run_case(0, c0, c1, x, w, b, (0, 0), relu=True)  # the forward's epilogue
    assert np.array_equal(got, np.maximum(want32, 0)) and (want32 < 0).any()
    if c1:  # the sources are told apart: the other order is another result
        other = np.concatenate([x[..., c0:], x[..., :c0]], -1)
        assert not np.array_equal(R.ref_layer(0, other, w, b), want32)


@gpu
@pytest.mark.parametrize("case", UP_CASES, ids=_id)
def test_upconv_exact(ivxlib, case):
    """ConvTranspose3d without ReLU, all eight output parity classes (each voxel of the 2S output belongs to one)"""
    _exact(ivxlib, (1,) + case)


@gpu
@pytest.mark.parametrize("case", REAL_CASES, ids=_id)
def test_tile_shapes_give_the_same_bits(ivxlib, case):
    """On real-valued data every tile shape runs the same ordered chain per output, so the bits agree; (1, 1) is within
    the worst-case bound of an ordered float32 sum of K products, (K + 1) 2^-23 (conv(|x|, |w|) + |b|): 2^-23 per
    operation rather than 2^-24 because the rounding inside a 4-term matrix-core step is not pinned down here."""
    kind, c0, c1, cout = case[:4]
    x, w, b, want, mag = case_data(*case, real=True)
    K = (125 if kind == 0 else 8) * (c0 + c1)  # a transposed conv's output sees 2^3 of the 4^3 taps
    base, _ = run_case(kind, c0, c1, x, w, b, (1, 1))
    err = np.abs(base.astype(np.float64) - want)
    print("max err / bound = %.3g" % float((err / ((K + 1) * 2.0 ** -23 * mag)).max()))
    assert (err <= (K + 1) * 2.0 ** -23 * mag).all()
    for tile in R.allowed_tiles(cout)[1:] + [(0, 0)]:
        got, _ = run_case(kind, c0, c1, x, w, b, tile)
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), tile


@gpu
@pytest.mark.parametrize("S", [2, 4, 6])
@pytest.mark.parametrize("C", [8, 64])
def test_pool_exact(ivxlib, S, C):
    from invesalius3_amd import segment as sg
    rng = np.random.default_rng([S, C])
    x = rng.standard_normal((3, S, S, S, C)).astype(np.float32)
    x[rng.random(x.shape) < 0.1] = -0.0
    x[rng.random(x.shape) < 0.1] = 0.0
    x[0, :2, :2, :2, 0] = -np.abs(x[0, :2, :2, :2, 0]) - 1  # a window of negative values only
    x[1, :2, :2, :2, 1] = -0.0
    want = np.stack([R.to_cl(R._pool(R.from_cl(p.astype(np.float64)))) for p in x]).astype(np.float32)
    assert (want < 0).any() and np.signbit(x).any()
    got = sg.pool_layer(x)
    assert got.shape == want.shape and np.array_equal(got, want)


@gpu
@pytest.mark.parametrize("nvox", [1, 255, 257])
def test_head_within_two_to_the_minus_22(ivxlib, nvox):
    """Integer activations and weights in eighths: the logit is exact in float32, so only expf (<= 1 ulp), one add and
    one divide separate p from the float64 sigmoid, and p <= 1."""
    from invesalius3_amd import segment as sg
    rng = np.random.default_rng(8)
    x = rng.integers(0, 8, (257, 8)).astype(np.float32)
    w = np.array([7, -5, 3, -8, 2, -1, 6, -4], np.float64) / 8
    x[254], x[256] = 7 * (w > 0), 7 * (w < 0)  # the two extreme logits, +-15.75 - 3/8
    b = -3 / 8
    s = x.astype(np.float64) @ w + b
    assert s.min() < -8 and s.max() > 8 and np.array_equal(s * 8, np.round(s * 8))
    x, s = x[:nvox], s[:nvox]
    got = sg.head_layer(x, w, b)
    assert got.dtype == np.float32 and got.shape == (nvox,)
    err = np.abs(got.astype(np.float64) - 1.0 / (1.0 + np.exp(-s)))
    print("max |dp| = %.3g" % float(err.max()))
    assert (err <= 2.0 ** -22).all()
