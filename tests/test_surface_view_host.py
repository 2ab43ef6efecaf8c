"""CPU: the surface view without a GPU -- the numpy restatement of rules R1 - R5 (tests/_surface_view_ref.py) against
hand-derived numbers, the camera from bounds against the camera of an image, the module's defaults against the reference's
constants, and csrc/surfview_math.h -- the very text the HIP kernels run -- compiled for the host and compared with the
restatement on every case: keys, ids, depth bits, float32 RGBA and RGBA8, all with np.array_equal (IEEE + - * / sqrt in one
order on both sides: there is nothing to tolerate)."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _surface_view_cases as C
import _surface_view_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the restatement against numbers derived by hand ---------------------------------------------------------------------------
def test_facing_triangle_has_intensity_one_and_its_exact_colour():
    colour = (0.33, 1.0, 0.33)
    verts, faces = C.hand_triangle()
    for mode, normals in ((R.FLAT, None), (R.GOURAUD, None), (R.GOURAUD, [[0, 0, 1]] * 3), (R.PHONG, [[0, 0, 1]] * 3)):
        out = R.render([R.layer(verts, faces, normals, colour)], C.hand_cam(), mode, background=(0.25, 0.5, 0.125))
        cov = {(int(i), int(j)) for j, i in zip(*np.nonzero(out["ids"][..., 0] >= 0))}
        assert cov == C.HAND_TRIANGLE_PIXELS  # centres on the three edges and on the three corners included
        for i, j in cov:
            assert np.array_equal(out["rgba"][j, i], np.array(colour + (1.0,), np.float32))
            assert tuple(out["ids"][j, i]) == (0, 0) and out["depth"][j, i] == np.float32(3.0)
        empty = out["ids"][..., 0] < 0
        assert (out["rgba"][empty] == np.array([0.25, 0.5, 0.125, 0.0], np.float32)).all()
        assert np.isposinf(out["depth"][empty]).all() and (out["ids"][empty] == -1).all()
        assert np.array_equal(out["rgba8"][2, 2], [84, 255, 84, 255]) and np.array_equal(out["rgba8"][0, 0], [64, 128, 32, 0])
    # the other winding faces away: nothing is drawn
    out = R.render([R.layer(verts, faces[:, ::-1], None, colour)], C.hand_cam())
    assert (out["keys"][0] == R.EMPTY).all() and (out["rgba"] == 0).all()


def test_depth_is_affine_on_the_screen():
    verts, faces = C.hand_triangle(t=(3.0, 1.0, 7.0))  # t = 3 at (2.5, 2.5), 1 at (2.5, 6.5), 7 at (6.5, 2.5)
    out = R.render([R.layer(verts, faces)], C.hand_cam())
    for i, j in C.HAND_TRIANGLE_PIXELS:
        assert out["depth"][j, i] == np.float32(3.0 + (i - 2) * 1.0 - (j - 2) * 0.5)


def test_triangle_tilted_by_sixty_degrees_has_intensity_one_half():
    s3 = 3.0 ** 0.5
    # the plane z = -sqrt(3) x: its normal (sqrt(3), 0, 1) / 2 makes 60 degrees with the direction to the viewer (0, 0, 1)
    verts = np.array([[-2, -2, 2 * s3], [2, -2, -2 * s3], [-2, 2, 2 * s3]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    n = [[s3 / 2, 0, 0.5]] * 3
    for mode, normals in ((R.FLAT, None), (R.GOURAUD, n), (R.PHONG, n)):
        out = R.render([R.layer(verts, faces, normals, (1.0, 0.5, 0.25))], C.hand_cam())
        hit = out["ids"][..., 0] == 0
        assert hit.sum() >= 6
        assert out["rgba"][hit][:, :3] == pytest.approx(np.tile([0.5, 0.25, 0.125], (hit.sum(), 1)), rel=1e-6)
        assert (out["rgba"][hit][:, 3] == 1.0).all()
    # normals that look away from the light give black, not a negative colour
    out = R.render([R.layer(verts, faces, [[0, 0, -1]] * 3, (1.0, 0.5, 0.25))], C.hand_cam(), R.GOURAUD)
    assert (out["rgba"][out["ids"][..., 0] == 0] == np.array([0, 0, 0, 1], np.float32)).all()
    out = R.render([R.layer(verts, faces, [[0, 0, 0]] * 3, (1.0, 0.5, 0.25))], C.hand_cam(), R.PHONG)  # a zero sum: I = 0
    assert (out["rgba"][out["ids"][..., 0] == 0] == np.array([0, 0, 0, 1], np.float32)).all()


def test_translucent_quarter_over_opaque():
    v1, f = C.hand_triangle(t=(3.0, 3.0, 3.0))
    v2, _ = C.hand_triangle(t=(5.0, 5.0, 5.0))
    front, back = R.layer(v1, f, None, (1.0, 0.5, 0.0), transparency=0.75), R.layer(v2, f, None, (0.0, 0.5, 1.0))
    for layers, nearest in (([front, back], 0), ([back, front], 1)):  # the order of the surfaces does not matter: depth does
        out = R.render(layers, C.hand_cam(), background=(1.0, 1.0, 1.0))
        for i, j in C.HAND_TRIANGLE_PIXELS:
            assert np.array_equal(out["rgba"][j, i], np.array([0.25, 0.5, 0.75, 1.0], np.float32))  # 0.25 c1 + 0.75 c2
            assert out["ids"][j, i, 0] == nearest and out["depth"][j, i] == np.float32(3.0)
    # the translucent one alone, over the background: C = 0.25 c + 0.75 bg, A = 0.25
    out = R.render([front], C.hand_cam(), background=(1.0, 1.0, 1.0))
    assert np.array_equal(out["rgba"][2, 2], np.array([1.0, 0.875, 0.75, 0.25], np.float32))
    # an opaque surface in front hides the translucent one behind it
    out = R.render([R.layer(v2, f, None, (1.0, 0.5, 0.0), transparency=0.75), R.layer(v1, f, None, (0.0, 0.5, 1.0))], C.hand_cam())
    assert np.array_equal(out["rgba"][2, 2], np.array([0.0, 0.5, 1.0, 1.0], np.float32)) and out["ids"][2, 2, 0] == 1


def test_shared_edge_and_coincident_triangles_go_to_the_lower_index():
    verts, faces = C.shared_edge_pair()
    out = R.render([R.layer(verts, faces)], C.hand_cam())
    tri = out["ids"][..., 1]
    want = np.full((16, 16), -1)
    for j in range(8, 13):
        for i in range(8, 13):
            want[j, i] = 0 if i >= j else 1  # the diagonal's centres lie on both triangles: exactly one wins, the lower id
    assert np.array_equal(tri, want)
    v, f = C.hand_triangle()
    out = R.render([R.layer(np.concatenate([v, v]), np.concatenate([f + 3, f]))], C.hand_cam())
    assert set(out["ids"][..., 1][out["ids"][..., 0] == 0].tolist()) == {0}
    # two identical surfaces: the lower surface index is in front
    out = R.render([R.layer(v, f, None, (1, 0, 0)), R.layer(v, f, None, (0, 0, 1))], C.hand_cam())
    assert np.array_equal(out["rgba"][2, 2], np.array([1, 0, 0, 1], np.float32)) and out["ids"][2, 2, 0] == 0


def test_ord_mapping_orders_negative_depths():
    vals = np.array([-np.inf, -7.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, np.inf], np.float32)
    o = R.ord_of(vals.view(np.uint32))
    assert (np.diff(o.astype(np.int64)) > 0).all()
    assert np.array_equal(R.bits_of(o), vals.view(np.uint32))
    out = R.render([R.layer(*C.tilted_sheet())], C.hand_cam((32, 32)))
    d = out["depth"][np.isfinite(out["depth"])]
    assert d.min() < -5.0 and d.max() > 5.0  # the sheet really crosses t = 0


def test_more_than_eight_surfaces_is_an_error():
    from invesalius3_amd import surface_view as SV
    with pytest.raises(TypeError):
        R.render(C.eight_layers(9), C.hand_cam())
    actors = [SV.SurfaceActor(m["verts"], m["faces"], m["normals"], m["colour"], m["transparency"]) for m in C.eight_layers(9)]
    with pytest.raises(TypeError):  # raised before anything is sent to the device
        SV.render_surfaces(actors, C.hand_cam(), (16, 16))
    actors[3].visible = False  # eight VISIBLE surfaces are fine for the check (the render itself needs a device)
    assert sum(a.visible for a in actors) == 8


# ---- camera and defaults ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", C.VIEW_NAMES)
@pytest.mark.parametrize("shape,spacing,size", [((40, 64, 48), (0.5, 0.75, 2.0), (96, 48)), ((7, 300, 11), (1.0, 1.0, 1.0), (512, 512)),
                                               ((1, 1, 1), (1.0, 1.0, 1.0), (3, 5))])
def test_camera_for_bounds_equals_camera_for_view(view, shape, spacing, size):
    from invesalius3_amd import surface_view as SV
    from invesalius3_amd import volume as V
    a, b = V.camera_for_view(view, shape, spacing, size), SV.camera_for_bounds(view, V.volume_bounds(shape, spacing), size)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_defaults_are_the_references():
    from invesalius3_amd import surface_view as SV
    ref = json.load(open(os.path.join(HERE, "golden", "ref_surfaceview.json")))
    assert SV.SURFACE_TRANSPARENCY == ref["SURFACE_TRANSPARENCY"] and SV.SURFACE_INTERPOLATION == ref["SURFACE_INTERPOLATION"]
    assert [list(map(float, c)) for c in SV.SURFACE_COLOUR] == ref["SURFACE_COLOUR"]
    a = SV.SurfaceActor(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert a.colour == tuple(ref["SURFACE_COLOUR"][0]) and a.transparency == 0.0 and a.visible
    assert SV.INTERPOLATIONS == {"flat": 0, "gouraud": 1, "phong": 2}


def test_c_structs_have_the_headers_layout():
    from invesalius3_amd import surface_view as SV
    assert ctypes.sizeof(SV.SurfaceCamera) == 112 and ctypes.sizeof(SV.SurfaceLayer) == 64
    assert SV.SurfaceLayer.keys.offset == 40 and SV.SurfaceLayer.rgb.offset == 48 and SV.SurfaceLayer.opacity.offset == 60


# ---- the kernels' arithmetic, compiled for the host --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_emu(tmp_path_factory):
    """tests/surfview_host_emu.cpp: csrc/surfview_math.h built with the host compiler, contraction off"""
    from invesalius3_amd import surface_view as SV
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("surfview_emu")
    exe = str(tmp / "emu")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "surfview_host_emu.cpp")], check=True)

    def run(layers, cam, mode, background):
        src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
        with open(src, "wb") as fh:
            fh.write(bytes(SV._c_camera(cam)) + np.array([len(layers), mode], np.int64).tobytes() + np.asarray(background, np.float32).tobytes())
            for m in layers:
                fh.write(np.array([len(m["verts"]), len(m["faces"]), m["normals"] is not None], np.int64).tobytes())
                fh.write(np.array(list(m["colour"]) + [m["opacity"]], np.float32).tobytes())
                fh.write(m["verts"].tobytes() + m["faces"].tobytes() + (b"" if m["normals"] is None else m["normals"].tobytes()))
        subprocess.run([exe, src, dst], check=True)
        W, H = cam["viewport"]
        raw, off, out = open(dst, "rb").read(), 0, {"keys": []}
        for _ in layers:
            out["keys"].append(np.frombuffer(raw, np.uint64, W * H, off).reshape(H, W))
            off += 8 * W * H
        for name, dt, per in (("rgba", np.float32, 4), ("rgba8", np.uint8, 4), ("ids", np.int32, 2), ("depth", np.float32, 1)):
            out[name] = np.frombuffer(raw, dt, W * H * per, off).reshape((H, W, per) if per > 1 else (H, W))
            off += W * H * per * np.dtype(dt).itemsize
        assert off == len(raw)
        return out
    return run


def assert_same_picture(got, want, name):
    assert len(got["keys"]) == len(want["keys"]), name
    for a, b in zip(got["keys"], want["keys"]):
        assert np.array_equal(a, b), name
    assert np.array_equal(got["ids"], want["ids"]), name
    assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32)), name
    assert np.array_equal(got["rgba"].view(np.uint32), want["rgba"].view(np.uint32)), name
    assert np.array_equal(got["rgba8"], want["rgba8"]), name


BACKGROUND = (0.125, 0.25, 0.5)


def test_kernel_arithmetic_on_the_host_equals_the_restatement(host_emu):
    """every key, id, depth bit and colour bit of every case, in all three interpolation modes: the C++ text of the rules and the
    numpy text of the rules are the same function"""
    drawn = 0
    for scene in C.scenes():
        for mode in (R.FLAT, R.GOURAUD, R.PHONG):
            want = R.render(scene["layers"], scene["cam"], mode, BACKGROUND)
            assert_same_picture(host_emu(scene["layers"], scene["cam"], mode, BACKGROUND), want, "%s mode %d" % (scene["name"], mode))
            drawn += int((want["ids"][..., 0] >= 0).any())
    assert drawn > 100


def test_shuffled_triangle_order_gives_the_same_picture(host_emu):
    """the cases without depth ties: the keys hold the same triangles whatever order they come in"""
    rng = np.random.default_rng(7)
    n = 0
    for scene in C.scenes():
        if scene["ties"] or not scene["layers"]:
            continue
        want = R.render(scene["layers"], scene["cam"], R.GOURAUD, BACKGROUND)
        perms = [rng.permutation(len(m["faces"])) for m in scene["layers"]]
        shuffled = [dict(m, faces=np.ascontiguousarray(m["faces"][p])) for m, p in zip(scene["layers"], perms)]
        got = host_emu(shuffled, scene["cam"], R.GOURAUD, BACKGROUND)
        ids = got["ids"].copy()
        for k, p in enumerate(perms):
            sel = ids[..., 0] == k
            ids[..., 1][sel] = p[ids[..., 1][sel]]
        assert np.array_equal(ids, want["ids"]), scene["name"]
        assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32)), scene["name"]
        assert np.array_equal(got["rgba"].view(np.uint32), want["rgba"].view(np.uint32)), scene["name"]
        n += 1
    assert n >= 30


def test_cases_cover_what_they_are_meant_to():
    by_name = {s["name"]: s for s in C.scenes()}
    def boxes(s):
        m, cam = s["layers"][0], s["cam"]
        X, Y, _, fin = R.project(m["verts"], cam)
        ok, x0, x1, y0, y1, _ = R.pixel_boxes(X, Y, fin, m["faces"], cam["viewport"])
        return ok, (x1 - x0 + 1) * (y1 - y0 + 1)
    for bw, bh in ((8, 8), (64, 1), (65, 1), (1, 65)):
        ok, box = boxes(by_name["box %d x %d" % (bw, bh)])
        assert ok.all() and box[0] == bw * bh  # 64 = the limit of the lane-per-triangle kernel, 65 one above
    ok, box = boxes(by_name["cube 256"])
    assert ok.sum() == 6 and (box[ok] > 64).all()  # the iso view sees three faces, all on the workgroup-per-triangle path
    ok, box = boxes(by_name["icosphere iso"])
    assert 600 < ok.sum() < 680 and len(ok) == 1280
    assert not boxes(by_name["wholly outside"])[0].any()
    ok, _ = boxes(by_name["partly outside"])
    assert 0 < ok.sum()
    part = R.render(by_name["partly outside"]["layers"], by_name["partly outside"]["cam"])
    assert (part["ids"][-1, :, 0] >= 0).any() or (part["ids"][:, -1, 0] >= 0).any() or (part["ids"][0, :, 0] >= 0).any() or (part["ids"][:, 0, 0] >= 0).any()
    deg = by_name["degenerate"]["layers"][0]
    good = R.render([dict(deg, faces=np.ascontiguousarray(deg["faces"][[q for q in range(len(deg["faces"])) if q not in (0, 41, 42, 43, len(deg["faces"]) - 1)]]))],
                    by_name["degenerate"]["cam"])
    both = R.render([deg], by_name["degenerate"]["cam"])
    assert np.array_equal(both["rgba"], good["rgba"]) and (both["ids"][..., 0] >= 0).any()  # the degenerate ones drew nothing
    for name in ("opaque inside translucent iso", "translucent inside opaque iso", "eight surfaces"):
        out = R.render(by_name[name]["layers"], by_name[name]["cam"])
        assert len(np.unique(out["rgba"].reshape(-1, 4), axis=0)) > 50
    inside = R.render(by_name["opaque inside translucent iso"]["layers"], by_name["opaque inside translucent iso"]["cam"])
    assert inside["rgba"][32, 32, 0] > 0.1 and inside["ids"][32, 32, 0] == 0  # the red ball shows through the green shell in front
    hidden = R.render(by_name["translucent inside opaque iso"]["layers"], by_name["translucent inside opaque iso"]["cam"])
    assert (hidden["ids"][..., 0] != 0).all()  # the inner ball is never the nearest, and never seen
    assert by_name["viewport 1 x 1"]["cam"]["viewport"] == (1, 1) and by_name["viewport 257 x 3"]["cam"]["viewport"] == (257, 3)
