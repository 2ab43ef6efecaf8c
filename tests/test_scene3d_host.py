"""CPU: the 3-D scene without a GPU -- the numpy restatement of rules S1 - S3 (tests/_scene3d_ref.py) against
hand-derived numbers, S1's claim that a surface's depth and a ray's distance are one axis, and csrc/scene3d_math.h -- the very
text the HIP kernel runs -- compiled for the host and compared with the restatement on every case: plane hits, texture samples,
K_f and the fragment order, all with np.array_equal."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _scene3d_cases as C
import _scene3d_ref as R3
import _surface_view_ref as SR

HERE = os.path.dirname(os.path.abspath(__file__))
VIEWS = ("front", "back", "right", "left", "top", "bottom", "iso")


def hand_scene(alpha_sample, shape=(5, 5, 5), size=(8, 8), dt=0.5):
    """a uniform field whose every sample has the colour (1, 0.5, 0.25) and the opacity `alpha_sample`, seen from the front with
    unit spacing: the rays enter at tin = -2 and take the samples k = 0 .. 8 at t = -2 + k / 2"""
    from invesalius3_amd import scene3d as S3
    cam = C.camera("front", shape, (1.0, 1.0, 1.0), size)
    _, setup = S3.field_setup(cam, (1.0, 1.0, 1.0), (0, 0), C.simple_preset(10.0, 100.0, background=(1.0, 1.0, 1.0)), sample_distance=dt)
    setup["rgba"] = np.tile([1.0, 0.5, 0.25, alpha_sample], (len(setup["alpha"]), 1))
    return cam, setup, np.zeros(shape, np.uint16)


def covered(layer, cam):
    return SR.raster_keys(layer["verts"], layer["faces"], cam) != SR.EMPTY


# ---- the restatement against numbers derived by hand ---------------------------------------------------------------------------
def test_opaque_quad_at_mid_depth_of_a_uniform_field():
    a = 0.125
    cam, setup, field = hand_scene(a)
    quad = SR.layer(*C.facing_quad(cam, 0.0, (1.0, 1.0)), colour=(0.25, 0.5, 1.0))
    out = R3.render(field, (1.0, 1.0, 1.0), setup, [quad], cam, SR.FLAT)
    on = covered(quad, cam)
    assert on.sum() >= 4 and not on.all()
    q4 = (1.0 - a) ** 4  # four samples lie in front of t = 0: k = 0 .. 3, K_f = 4
    want = np.array([1.0, 0.5, 0.25]) * (1.0 - q4) + q4 * np.array([0.25, 0.5, 1.0])
    assert (out["kf"][0].reshape(on.shape)[on] == 4).all()
    assert out["image"][on][:, :3] == pytest.approx(np.tile(want, (on.sum(), 1)), abs=1e-15)
    assert (out["image"][on][:, 3] == 1.0).all() and (out["taken"].reshape(on.shape)[on] == 4).all()
    # beside the quad the ray runs through: nine samples over the white background
    q9 = (1.0 - a) ** 9
    free = ~on & out["hit"].reshape(on.shape)
    assert free.any()
    assert out["image"][free][:, :3] == pytest.approx(np.tile(np.array([1.0, 0.5, 0.25]) * (1.0 - q9) + q9, (free.sum(), 1)), abs=1e-15)
    assert (out["taken"].reshape(on.shape)[free] == 9).all()


def test_translucent_quad_in_an_empty_field_is_the_plain_blend():
    cam, setup, field = hand_scene(0.0)
    quad = SR.layer(*C.facing_quad(cam, 0.0, (1.0, 1.0)), colour=(1.0, 0.5, 0.0), transparency=0.75)
    out = R3.render(field, (1.0, 1.0, 1.0), setup, [quad], cam, SR.FLAT)
    on = covered(quad, cam)
    assert on.any()
    assert (out["image"][on] == np.array([1.0, 0.875, 0.75, 0.25])).all()  # 0.25 c + 0.75 white, exactly
    assert (out["image"][~on] == np.array([1.0, 1.0, 1.0, 0.0])).all()


def test_plane_hit_at_a_corner_is_inside_and_a_ray_in_the_plane_hits_nothing():
    h, w, sp = 5, 7, (1.0, 1.0, 1.0)
    corners = np.array([[0.0, 0.0, -3.0], [w - 1.0, 0.0, -3.0], [0.0, -(h - 1.0), -3.0], [w - 1.0, -(h - 1.0), -3.0]])
    hit, t, u, v = R3.plane_hit(corners, (0.0, 0.0, 1.0), sp, "AXIAL", 2, h, w)
    assert hit.all() and (t == np.float32(5.0)).all()
    assert np.array_equal(u, np.array([0, w - 1, 0, w - 1], np.float32)) and np.array_equal(v, np.array([0, 0, h - 1, h - 1], np.float32))
    outside = np.array([[-2.0 ** -40, 0.0, -3.0], [w - 1.0 + 2.0 ** -30, 0.0, -3.0], [0.0, 2.0 ** -40, -3.0],
                        [w - 1.0, -(h - 1.0) - 2.0 ** -30, -3.0]])  # one step past each side
    assert not R3.plane_hit(outside, (0.0, 0.0, 1.0), sp, "AXIAL", 2, h, w)[0].any()
    # dir[a] == 0: the ray runs in (or beside) the plane
    for o, d in (("AXIAL", (1.0, 0.0, 0.0)), ("CORONAL", (0.0, 0.0, 1.0)), ("SAGITAL", (0.0, 1.0, 0.0))):
        assert not R3.plane_hit(np.array([[1.0, -1.0, 2.0]]), d, sp, o, 2, h, w)[0].any()
    # the other two orientations, and the padded matrix's frame (off = 1: the same plane, the same point)
    hit, t, u, v = R3.plane_hit(np.array([[3.0, -9.0, 2.0]]), (0.0, 1.0, 0.0), sp, "CORONAL", 4, 6, w)
    assert hit[0] and t[0] == 5.0 and (u[0], v[0]) == (3.0, 2.0)
    hit, t, u, v = R3.plane_hit(np.array([[-4.0, -1.0, 2.0]]), (1.0, 0.0, 0.0), sp, "SAGITAL", 3, 6, h)
    assert hit[0] and t[0] == 7.0 and (u[0], v[0]) == (1.0, 2.0)
    hit, t, u, v = R3.plane_hit(np.array([[-3.0, -2.0, 3.0]]), (1.0, 0.0, 0.0), sp, "SAGITAL", 3, 6, h, off=1)
    assert hit[0] and t[0] == 7.0 and (u[0], v[0]) == (1.0, 2.0)


def test_texture_sample_is_bilinear_with_clamped_ends():
    pic = np.zeros((2, 3, 3), np.uint8)
    pic[0, :, 0], pic[1, :, 0] = [0, 100, 200], [50, 150, 250]
    got = R3.texel(pic, np.array([0.0, 0.5, 2.0, 1.25], np.float32), np.array([0.0, 0.5, 1.0, 0.0], np.float32))[:, 0]
    assert np.array_equal(got, np.array([0.0, 75.0, 250.0, 125.0], np.float32) / np.float32(255.0))
    one = np.full((1, 1, 3), 51, np.uint8)
    assert np.array_equal(R3.texel(one, np.zeros(1, np.float32), np.zeros(1, np.float32)), np.full((1, 3), np.float32(51.0) / np.float32(255.0)))


def test_fragment_on_a_sample_goes_before_it():
    case = C.exact_sample_case()
    ref = C.reference(case)
    on = covered(case["layers"][0], case["cam"]).ravel()
    assert on.any() and (ref["kf"][0][on] == 13).all()  # t = 2.0 = -4.5 + 13 * 0.5
    assert R3.frag_sample(np.float32(2.0), -4.5, 0.5, 18) == 13
    assert R3.frag_sample(np.nextafter(np.float32(2.0), np.float32(3.0)), -4.5, 0.5, 18) == 14
    assert R3.frag_sample(np.float32(-100.0), -4.5, 0.5, 18) == 0 and R3.frag_sample(np.float32(100.0), -4.5, 0.5, 18) == 19
    assert R3.frag_sample(np.float32(1.0), 0.0, 0.5, -1) == 0  # a ray without samples


def test_fragment_order_is_depth_then_layer():
    sk = np.full((R3.MAX_FRAGS, 2), R3.EMPTY, np.uint64)
    for layer, t in ((0, 3.0), (5, -1.0), (8, 3.0), (10, -0.0), (2, 0.0)):
        sk[layer, 0] = R3.frag_key(np.float32(t), layer)
    order = R3.frag_order(sk)
    assert list(order[:, 0]) == [5, 10, 2, 0, 8] + [-1] * 6 and (order[:, 1] == -1).all()  # (-0 sorts just below +0)


# ---- S1: one depth axis ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", VIEWS)
def test_surface_depth_and_ray_distance_are_one_axis(view):
    from invesalius3_amd import volume as V
    from invesalius3_amd import volume_mask as VM
    import _volren_ref as R
    shape, sp, size = C.SHAPES["small"], C.SPACING, (19, 13)
    cam = C.camera(view, shape, sp, size)
    f, r, u, d = C.cam_frame(cam)
    image_setup = V.render_setup(C.HAZE_PRESET, (-1024, 3071), cam)
    mask_setup = VM.render_setup((1.0, 0.0, 0.0), "composite", cam, sp)
    rng = np.random.default_rng(5)
    rows, cols = rng.integers(0, size[1], 40), rng.integers(0, size[0], 40)
    ts = rng.uniform(-12.0, 12.0, 40)
    scale = np.abs(f).max() + 12.0
    shift = np.array([sp[0], -sp[1], sp[2]])
    padded = tuple(s + 1 for s in shape)
    for setup, fshape, move in ((image_setup, shape, 0.0), (mask_setup, padded, 1.0)):
        P0 = R3.pixel_origins(setup, (rows, cols))
        # the pixel plane passes through the focal point (moved with the origin for the mask): P0 - focal is orthogonal to dir
        assert np.abs((P0 - move * shift - f) @ d).max() <= 8 * np.finfo(np.float64).eps * scale
        A, B, hi, tin, kmax = R.rays(fshape, sp, setup, (rows, cols))
        for k in range(40):
            world = P0[k] - move * shift + ts[k] * d  # the point at distance t of the ray, in the image's world
            # the surface pass gives it the same depth (float32 of a float64 that differs by rounding alone)
            assert abs(float(R3.surface_t(cam, world.astype(np.float32).astype(np.float64))) - ts[k]) <= 4 * np.finfo(np.float32).eps * scale
            # and the ray's index position at t is the point's voxel index (plus one on the padded matrix)
            index = np.array([world[0] / sp[0], -world[1] / sp[1], world[2] / sp[2]]) + move
            assert np.abs(A[k] + ts[k] * B - index).max() <= 64 * np.finfo(np.float64).eps * scale


# ---- the kernel's arithmetic, compiled for the host ---------------------------------------------------------------------------------
HIT = np.dtype([("P0", "<f8", 3), ("dir", "<f8", 3), ("spacing", "<f8", 3), ("orientation", "<i4"), ("slice", "<i4"), ("h", "<i4"),
                ("w", "<i4"), ("off", "<i4"), ("pad", "<i4")])
KF = np.dtype([("tin", "<f8"), ("dt", "<f8"), ("kmax", "<i8"), ("t", "<f4"), ("pad", "<i4")])
HIT_OUT = np.dtype([("hit", "<i4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4")])


@pytest.fixture(scope="module")
def host_emu(tmp_path_factory):
    """tests/scene3d_host_emu.cpp: csrc/scene3d_math.h built with the host compiler, contraction off"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("scene3d_emu")
    exe = str(tmp / "emu")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "scene3d_host_emu.cpp")], check=True)

    def run(hits, textures, kfs, sks):
        src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
        with open(src, "wb") as fh:
            fh.write(np.array([len(hits), len(textures), len(kfs), len(sks)], np.int64).tobytes())
            fh.write(hits.tobytes())
            for pic, uv in textures:
                fh.write(np.array([pic.shape[0], pic.shape[1], len(uv)], np.int64).tobytes() + pic.tobytes() + uv.astype(np.float32).tobytes())
            fh.write(kfs.tobytes() + np.ascontiguousarray(sks, np.uint64).tobytes())
        subprocess.run([exe, src, dst], check=True)
        raw, off = open(dst, "rb").read(), 0
        out_hits = np.frombuffer(raw, HIT_OUT, len(hits), off)
        off += HIT_OUT.itemsize * len(hits)
        out_tex = []
        for pic, uv in textures:
            out_tex.append(np.frombuffer(raw, np.float32, 3 * len(uv), off).reshape(-1, 3))
            off += 12 * len(uv)
        out_kf = np.frombuffer(raw, np.int64, len(kfs), off)
        off += 8 * len(kfs)
        out_ord = np.frombuffer(raw, np.int32, R3.MAX_FRAGS * len(sks), off).reshape(-1, R3.MAX_FRAGS)
        assert off + out_ord.nbytes == len(raw)
        return out_hits, out_tex, out_kf, out_ord

    return run


def test_kernel_arithmetic_on_the_host_equals_the_restatement(host_emu):
    import _volren_ref as R
    n_hits = n_frags = 0
    for case in C.cases():
        field, setup = C.setup_of(case)
        off = 1 if case["kind"] == R3.MASK else 0
        P0 = R3.pixel_origins(setup)
        n = len(P0)
        hits, textures, want_hits, want_tex = [], [], [], []
        for p in case["planes"]:
            h, w = p["picture"].shape[:2]
            q = np.zeros(n, HIT)
            q["P0"], q["dir"], q["spacing"] = P0, np.asarray(setup["dir"], np.float64), case["spacing"]
            q["orientation"], q["slice"], q["h"], q["w"], q["off"] = R3.ORIENTATIONS[p["orientation"]], p["n"], h, w, off
            hits.append(q)
            hit, t, u, v = R3.plane_hit(P0, setup["dir"], case["spacing"], p["orientation"], p["n"], h, w, off)
            want_hits.append((hit, t, u, v))
            uv = np.stack([u[hit], v[hit]], 1)
            textures.append((p["picture"], uv))
            want_tex.append(R3.texel(p["picture"], u[hit], v[hit]))
            n_hits += int(hit.sum())
        sk, _, _ = R3.fragments(setup, case["spacing"], case["layers"], case["cam"], case["mode"], case["planes"], off)
        if case["kind"] == R3.NONE:
            tin, kmax = np.zeros(n), np.full(n, -1, np.int64)
        else:
            _, _, _, tin, kmax = R.rays(field.shape, case["spacing"], setup)
            tin = np.where(kmax >= 0, tin, 0.0)
        lay, ray = np.nonzero(sk != R3.EMPTY)
        kfs = np.zeros(len(lay), KF)
        kfs["tin"], kfs["dt"], kfs["kmax"], kfs["t"] = tin[ray], setup["dt"], kmax[ray], R3.key_depth(sk[lay, ray])
        n_frags += len(lay)
        got_hits, got_tex, got_kf, got_ord = host_emu(np.concatenate(hits) if hits else np.zeros(0, HIT), textures, kfs, sk.T)
        for k, (hit, t, u, v) in enumerate(want_hits):
            g = got_hits[k * n:(k + 1) * n]
            assert np.array_equal(g["hit"] != 0, hit), case["name"]
            for name, want in (("t", t), ("u", u), ("v", v)):
                assert np.array_equal(g[name][hit].view(np.uint32), want[hit].view(np.uint32)), (case["name"], name)
            assert np.array_equal(got_tex[k].view(np.uint32), want_tex[k].view(np.uint32)), case["name"]
        ref = C.reference(case)
        assert np.array_equal(got_kf, ref["kf"][lay, ray]), case["name"]
        assert np.array_equal(got_ord.T, ref["order"]), case["name"]
    assert n_hits > 1000 and n_frags > 3000
