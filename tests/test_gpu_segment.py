"""The U-Net brain / trachea segmentation on the GPU (segment.py, k_unet.hip) against the three-layer contract:
the forward within 5e-5 of a float64 restatement, the pipeline bit-equal to numpy's in-order accumulation over the
forward's outputs, the threshold exact.  torch is never imported here (tests/_unet_ref.py restates the network)."""
import os

import numpy as np
import pytest

import _unet_ref as R

pytestmark = pytest.mark.gpu

BOUND = 5e-5
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def sd():
    return R.make_weights()


@pytest.fixture(scope="module")
def net(ivxlib, sd):
    from invesalius3_amd import segment as sg
    n = sg.Unet3D(sd)
    yield n
    n.close()


def _patches(P, n, seed):
    from invesalius3_amd.segment import image_normalize_f32
    return np.stack([image_normalize_f32(R.ct_volume((P, P, P), seed + i)) for i in range(n)])


@pytest.mark.parametrize("P,n", [(16, 1), (16, 3), (32, 1), (32, 3), (48, 1), (48, 3)])
def test_forward_within_bound_of_float64(net, sd, P, n):
    x = _patches(P, n, 100 * P + n)
    got = net.forward(x)
    assert got.dtype == np.float32 and got.shape == x.shape
    err = max(float(np.abs(got[i].astype(np.float64) - R.forward64(sd, x[i])).max()) for i in range(n))
    print("P=%d n=%d max |dp| = %.3g" % (P, n, err))
    assert err <= BOUND


def test_forward_patch_count_off_the_batch_tile(net, sd):
    """37 patches through a workspace of 8: five chunks, the last one short"""
    x = _patches(16, 37, 7)
    got = net.forward(x, batch=8)
    want = np.stack([R.forward64(sd, p) for p in x])
    assert float(np.abs(got - want).max()) <= BOUND
    # chunking changes nothing: each patch's output is its own
    assert np.array_equal(got, net.forward(x, batch=37))


@pytest.fixture(scope="module")
def sixteen(net, sd):
    """16 distinct 16^3 patches, their forward in one batch of 16, and its distance from float64"""
    x = _patches(16, 16, 900)
    small = net.forward(x, batch=16)
    err = max(float(np.abs(small[i].astype(np.float64) - R.forward64(sd, x[i])).max()) for i in range(16))
    for a in (x, small):
        a.setflags(write=False)
    return x, small, err


@pytest.mark.parametrize("n", [1024, 2048])
def test_forward_in_one_large_batch_equals_small_batches(net, sixteen, n):
    """One batch of 1024 (2048) patches makes run_conv take the 2 x 2 (4 x 2) tiles for the 32-channel layers, which no
    smaller batch of 16^3 patches does; a patch's output is its own whatever the batch and the tile shape."""
    x, small, err = sixteen
    print("16 patches: max |dp| = %.3g" % err)
    assert err <= BOUND
    try:
        got = net.forward(np.tile(x, (n // 16, 1, 1, 1)), batch=n)
    except MemoryError:
        if n == 2048:  # a workspace of 0.9 GB
            pytest.skip("no room for the workspace of 2048 patches")
        raise
    assert np.array_equal(got.view(np.uint32), np.tile(small, (n // 16, 1, 1, 1)).view(np.uint32))


@pytest.mark.parametrize("n,tile", [(1024, (2, 2)), (2048, (4, 2))])
def test_run_conv_takes_the_big_tiles_for_the_32_channel_layers(ivxlib, n, tile):
    """The 32-channel layers of a 16^3 patch (edge 4) in one batch of n, each through the layer entry point with the
    forward's own choice of tile: if the rule is retuned this says that the test above lost its coverage.  Integer data:
    the first two and the last patch are compared exactly with float64."""
    from invesalius3_amd import segment as sg
    #        kind, c0, c1, edge of the input
    layers = [(0, 16, 0, 4), (0, 32, 0, 4), (1, 64, 0, 2), (0, 32, 32, 4)]  # enc3 conv1, 32 -> 32 convs, upconv3, dec3 conv1
    for kind, c0, c1, S in layers:
        assert R.pick_tile(kind, n * S ** 3, 32) == tile
        x, w, b = R.int_case(kind, c0, c1, 32, S, 16, [kind, c0, c1])
        x = np.tile(x, (n // 16, 1, 1, 1, 1))
        x[-1] = x[-1, ::-1]  # the last patch is like no other
        got, used = sg.conv_layer(kind, x[..., :c0], w, b, x[..., c0:] if c1 else None, relu=kind == 0)
        assert used == tile, (kind, c0, c1, used)
        sel = [0, 1, n - 1]
        want = R.ref_layer(kind, x[sel], w, b)
        assert np.array_equal(got[sel], (np.maximum(want, 0) if kind == 0 else want).astype(np.float32)), (kind, c0, c1)
        assert np.array_equal(got[16:32], got[:16])


@pytest.mark.parametrize("shape,P,overlap,batch", [((24, 40, 45), 32, 50, 32), ((24, 40, 45), 32, 50, 1),
                                                   ((20, 37, 30), 16, 25, 3), ((33, 18, 40), 16, 0, 5),
                                                   ((10, 12, 9), 16, 50, 2)])
def test_pipeline_bit_equal_to_in_order_accumulation(net, shape, P, overlap, batch):
    from invesalius3_amd import segment as sg
    img = R.ct_volume(shape, 11)
    want, _ = R.host_pipeline(net, img, P, overlap)
    got = sg.segment_unet3d(img, net, overlap, P, batch=batch)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_two_runs_bit_identical(net):
    from invesalius3_amd import segment as sg
    img = R.ct_volume((40, 44, 50), 5)
    a = sg.segment_unet3d(img, net, 50, 32)
    b = sg.segment_unet3d(img, net, 50, 32, batch=3)
    assert np.array_equal(a, b)


def test_accumulates_onto_the_callers_array_and_strided_image(net):
    from invesalius3_amd import segment as sg
    img = R.ct_volume((20, 30, 40), 8)
    view = np.asfortranarray(img)[:, ::-1][:, ::-1]  # non-C strides
    prob0 = np.random.default_rng(1).random(img.shape).astype(np.float32)
    from invesalius3_amd.segment import image_normalize_f32, gen_patches
    nrm = image_normalize_f32(img)
    outs = net.forward(np.stack([p.copy() for _, p, _ in gen_patches(nrm, 16, 50)]))
    want = R.accumulate(nrm, 16, 50, outs, prob0)
    got = prob0.copy()
    comm = np.zeros(1, np.float32)
    sg.segment_unet3d(view, net, 50, 16, probability_array=got, comm_array=comm)
    assert np.array_equal(got, want) and comm[0] == np.inf


@pytest.mark.parametrize("case", ["wrap", "wwwl", "constant"])
def test_normalisation_cases(net, case):
    from invesalius3_amd import segment as sg
    rng = np.random.default_rng(3)
    kw = {}
    if case == "wrap":  # range > 32767: image - imin and imax - imin both wrap in int16
        img = rng.integers(-20000, 20000, (20, 24, 28)).astype(np.int16)
        img[0, 0, 0], img[-1, -1, -1] = -20000, 20000
    elif case == "wwwl":
        img = R.ct_volume((20, 24, 28), 4)
        kw = dict(apply_wwwl=True, ww=400, wl=40)
    else:
        img = np.full((20, 24, 28), 123, np.int16)
    want, nrm = R.host_pipeline(net, img, 16, 50, **kw)
    if case == "constant":
        assert not nrm.any()
    if case == "wrap":
        assert nrm.min() < 0 or nrm.max() > 1  # the wrap is visible
    got = sg.segment_unet3d(img, net, 50, 16, apply_wwwl=bool(kw), window_width=kw.get("ww", 255),
                            window_level=kw.get("wl", 127))
    assert np.array_equal(got, want)


def _host_threshold(prob, mask0, thr):
    m = mask0.copy()
    m[1:, 1:, 1:] = (prob >= thr) * 255
    m[:, 0, 0] = 2
    m[0, :, 0] = 2
    m[0, 0, :] = 2
    return m


@pytest.mark.parametrize("thr", [0.7, 0.75, 0.3])
def test_threshold_exact_on_float32_neighbours(ivxlib, thr):
    from invesalius3_amd import segment as sg
    t = np.float32(thr)
    vals = np.array([np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1)), thr, 0.0, 1.0], np.float32)
    rng = np.random.default_rng(9)
    prob = vals[rng.integers(0, vals.size, (9, 10, 11))]
    mask0 = rng.integers(0, 256, (10, 11, 12)).astype(np.uint8)  # border planes must keep their bytes
    got = sg.apply_segment_threshold(mask0.copy(), prob, thr)
    assert np.array_equal(got, _host_threshold(prob, mask0, thr))
    if thr == 0.7:  # f32(0.7) < 0.7: numpy keeps the voxel, a float64 comparison would drop it
        assert float(t) < 0.7 and (got[1:, 1:, 1:][prob == t] == 255).all()


def test_device_volume_segment_threshold_and_surface(net, oracle):
    from invesalius3_amd import segment as sg
    from invesalius3_amd.device import DeviceVolume
    img = R.ct_volume((30, 34, 38), 21)
    spacing = (0.5, 0.6, 1.0)
    prob = sg.segment_unet3d(img, net, 50, 16)
    with DeviceVolume(img, spacing=spacing) as vol:
        vol.segment_unet3d(net, overlap=50, patch_size=16)
        assert np.array_equal(vol.prob.download(img.shape, np.float32), prob)
        for thr in (0.75, 0.3):
            host = sg.apply_segment_threshold(np.zeros(tuple(s + 1 for s in img.shape), np.uint8), prob, thr)
            vol.apply_segment_threshold(thr)
            assert np.array_equal(vol.download_mask(), host[1:, 1:, 1:])
            assert 0 < (host[1:, 1:, 1:] == 255).sum() < img.size
            tris = vol.marching_cubes(from_binary=True, download=True)
            ref = oracle.marching_cubes(np.ascontiguousarray(host[1:, 1:, 1:]), spacing, [127.0], 0, True, True, True, 0.0, 1)
            assert tris.shape == ref.shape and np.array_equal(tris, ref)


def test_refusals(ivxlib, net, tmp_path):
    from invesalius3_amd import segment as sg
    img = np.zeros((8, 8, 8), np.int16)
    with pytest.raises(ValueError):
        sg.segment_unet3d(img, net, 50, 24)
    with pytest.raises(ValueError):
        sg.segment_unet3d(img, net, 100, 16)
    with pytest.raises(FileNotFoundError):
        sg.segment_torch(img, tmp_path / "missing.pt", 50, "cpu", np.zeros(img.shape, np.float32), np.zeros(1, np.float32), 16)


def test_pipeline_against_the_references_own_run(net):
    """tests/golden/ref_segment.npz: the reference's segment_torch on real torch (float32, CPU) with the same weights.
    The maps agree within the bound; the masks only differ where the reference's p is within the bound of f32(0.75)."""
    from invesalius3_amd import segment as sg
    with np.load(os.path.join(HERE, "golden", "ref_segment.npz")) as z:
        gold = {k: z[k] for k in z.files}
    thr = np.float32(0.75)
    for case in gold["seg_cases"]:
        name, P, ov, wwwl, ww, wl = str(case).split("|")
        vol, pref, mref = gold["vol_" + name], gold["prob_" + name], gold["mask_" + name]
        got = sg.segment_unet3d(vol, net, int(ov), int(P), apply_wwwl=bool(int(wwwl)), window_width=int(ww),
                                window_level=int(wl))
        err = float(np.abs(got.astype(np.float64) - pref).max())
        print("%s: max |p - p_ref| = %.3g" % (name, err))
        assert err <= BOUND, name
        m = sg.apply_segment_threshold(np.zeros_like(mref), got, 0.75)
        diff = m != mref
        assert not diff[0].any() and not diff[:, 0].any() and not diff[:, :, 0].any()
        assert (np.abs(pref[diff[1:, 1:, 1:]] - thr) <= BOUND).all(), name


def test_headless_segment_writes_stl_and_mask(ivxlib, net, tmp_path, capsys, sd):
    import json
    from invesalius3_amd import headless
    from invesalius3_amd import project as prj
    from invesalius3_amd import segment as sg
    img = R.ct_volume((40, 44, 52), 13)
    p = prj.Project(name="Synth", spacing=(0.5, 0.5, 1.0), threshold_range=(int(img.min()), int(img.max())))
    p.matrix = img
    src, w, stl, saved = tmp_path / "in.inv3", tmp_path / "W.npz", tmp_path / "seg.stl", tmp_path / "out.inv3"
    prj.save_inv3(src, p)
    np.savez(w, **sd)
    argv = [src, "--segment", "brain", "--weights", w, "--overlap", "25", "--seg-threshold", "0.7", "--stl", stl,
            "--save", saved]
    assert headless.main([str(a) for a in argv]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["segment"]["tool"] == "brain_mri_t1" and res["surface"]["triangles"] > 0
    assert open(stl, "rb").read(84)[80:] != b"\0\0\0\0"
    # SegmentProcess for patch 48: the host path gives the same mask
    prob = sg.segment_unet3d(img, net, 25, 48)
    want = sg.apply_segment_threshold(np.zeros(tuple(s + 1 for s in img.shape), np.uint8), prob, 0.7)
    r = prj.open_inv3(saved)
    try:
        got = r.masks[max(r.masks)].matrix
        assert np.array_equal(np.asarray(got), want)
    finally:
        r.close()
