"""CPU: the host side of the surface visibility tools -- the cameras `polydata_utils.views_for_positions` builds,
against hand-derived numbers, and self-checks of the numpy restatement the GPU tests compare with (tests/_meshvis_ref.py)."""
import math

import numpy as np
import pytest

import _meshvis_cases as C
import _meshvis_ref as R

BOX = (10.0, 13.0, -20.0, -15.0, 100.0, 107.0)  # extents 3 : 5 : 7, off the origin
CENTRE = (11.5, -17.5, 103.5)
SIN15 = (math.sqrt(6.0) - math.sqrt(2.0)) / 4.0
DIST = math.sqrt(83.0) / 2.0 / SIN15            # radius = sqrt(9 + 25 + 49) / 2


def _views(positions=None, size=(800, 800)):
    from invesalius3_amd import polydata_utils as pu
    return pu.views_for_positions(BOX, pu.POSITIONS if positions is None else positions, size)


def test_default_positions_are_the_references_six_in_order():
    from invesalius3_amd import polydata_utils as pu
    assert [tuple(p) for p in pu.POSITIONS] == [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    assert pu.SIZE == (800, 800)


def test_eyes_and_distance_of_an_asymmetric_box():
    views = _views()
    assert len(views) == 6
    want = [(CENTRE[0] + DIST, CENTRE[1], CENTRE[2]), (CENTRE[0] - DIST, CENTRE[1], CENTRE[2]),
            (CENTRE[0], CENTRE[1] + DIST, CENTRE[2]), (CENTRE[0], CENTRE[1] - DIST, CENTRE[2]),
            (CENTRE[0], CENTRE[1], CENTRE[2] + DIST), (CENTRE[0], CENTRE[1], CENTRE[2] - DIST)]
    for v, eye in zip(views, want):
        assert v["dist"] == pytest.approx(DIST, rel=1e-14) and v["dist"] == pytest.approx(17.600003, rel=1e-6)
        assert v["eye"] == pytest.approx(eye, rel=1e-14)
        assert v["centre"] == list(CENTRE)
        assert v["tan_half"] == pytest.approx(2.0 - math.sqrt(3.0), rel=1e-14) and v["aspect"] == 1.0
        # an orthonormal, right-handed frame looking at the centre
        r, u, f = (np.array(v[k]) for k in ("right", "up", "fwd"))
        assert np.allclose([r @ r, u @ u, f @ f, r @ u, r @ f, u @ f], [1, 1, 1, 0, 0, 0], atol=1e-15)
        assert np.allclose(np.cross(r, u), -f, atol=1e-15)
        assert np.allclose(np.array(v["eye"]) + f * v["dist"], CENTRE, atol=1e-12)


def test_view_up_is_carried_along_the_list():
    ups = [tuple(abs(x) if x == 0 else x for x in v["view_up"]) for v in _views()]
    assert ups == [(0, 1, 0), (0, 1, 0), (0, 0, 1), (0, 0, 1), (-1, 0, 0), (-1, 0, 0)]
    # the turn stays: a list that starts with +y then goes back to +x keeps (0, 0, 1)
    ups = [tuple(abs(x) if x == 0 else x for x in v["view_up"]) for v in _views([(0, 1, 0), (1, 0, 0)])]
    assert ups == [(0, 0, 1), (0, 0, 1)]
    # screen up of the +x view is +y, of the +y view +z, of the +z view -x
    views = _views()
    assert np.allclose(views[0]["up"], (0, 1, 0)) and np.allclose(views[2]["up"], (0, 0, 1)) and np.allclose(views[4]["up"], (-1, 0, 0))


def test_non_axis_position():
    (v,) = _views([(1, 1, 1)], (96, 48))
    n = np.ones(3) / math.sqrt(3.0)
    assert np.allclose(v["eye"], np.array(CENTRE) + n * DIST, rtol=1e-14)
    assert np.allclose(v["fwd"], -n, rtol=1e-15)
    assert v["view_up"] == [0.0, 1.0, 0.0] and v["aspect"] == 2.0
    right = np.cross(-n, (0, 1, 0))
    right /= np.linalg.norm(right)
    assert np.allclose(v["right"], right, atol=1e-15) and np.allclose(v["up"], np.cross(right, -n), atol=1e-15)
    # a position is a direction: its length does not matter
    (v2,) = _views([(5, 5, 5)], (96, 48))
    assert np.allclose(v2["eye"], v["eye"], rtol=1e-14)


@pytest.mark.parametrize("positions", [None, [(1, 1, 1)], [(-2, 1, 0.5)]])
def test_clipping_range_against_the_formula_on_the_corners(positions):
    corners = np.array([[x, y, z] for x in BOX[0:2] for y in BOX[2:4] for z in BOX[4:6]])
    for v in _views(positions):
        d = (corners - np.array(v["eye"])) @ np.array(v["fwd"])
        n0, f0 = d.min(), d.max()
        near = 0.99 * n0 - 0.5 * (f0 - n0)
        far = 1.01 * f0 + 0.5 * (f0 - near)
        assert near < far and near > 0.001 * far
        assert v["near"] == pytest.approx(near, rel=1e-13) and v["far"] == pytest.approx(far, rel=1e-13)
        assert v["near"] < n0 and v["far"] > f0
    # the +x view by hand: the corners lie dist -+ 1.5 in front of the eye
    v = _views()[0]
    assert v["near"] == pytest.approx(0.99 * (DIST - 1.5) - 1.5, rel=1e-13)
    assert v["far"] == pytest.approx(1.01 * (DIST + 1.5) + 0.5 * ((DIST + 1.5) - v["near"]), rel=1e-13)


def test_degenerate_bounds():
    from invesalius3_amd import polydata_utils as pu
    for v in pu.views_for_positions((2.0, 2.0, 3.0, 3.0, 4.0, 4.0)):  # one point: radius 1
        assert v["dist"] == pytest.approx(1.0 / SIN15, rel=1e-14)
        assert 0.0 < v["near"] < v["far"] and v["near"] >= 0.001 * v["far"]
    with pytest.raises(ValueError):
        pu.views_for_positions(BOX, size=(0, 10))


@pytest.mark.parametrize("size", [(800, 800), (48, 96), (96, 48)])
def test_every_corner_projects_inside_the_square_viewport_and_the_clipping_range(size):
    corners = np.array([[x, y, z] for x in BOX[0:2] for y in BOX[2:4] for z in BOX[4:6]], np.float32)
    for v in _views(None, size) + _views([(1, 1, 1)], size):
        xs, ys, zw, front = R.project(corners, v)
        assert front.all() and (zw > 0).all() and (zw < 1).all()
        if size == (800, 800):
            assert (xs > 0).all() and (xs < 800).all() and (ys > 0).all() and (ys < 800).all()
        else:  # the vertical angle is fixed: the tall side always fits
            assert (ys > 0).all() and (ys < size[1]).all()


def test_product_cameras_equal_the_restatement_bit_for_bit():
    for positions, size in ((R.POSITIONS, (800, 800)), ([(1, 1, 1), (0, 1, 0), (-3, 0.5, 2)], (48, 96))):
        for a, b in zip(_views(positions, size), R.views(BOX, positions, size)):
            for k in ("eye", "right", "up", "fwd", "near", "far", "tan_half", "aspect", "size"):
                assert a[k] == b[k], k


# ---- self-checks of the restatement --------------------------------------------------------------------------------------------
def test_oracle_hand_triangle_covers_the_pixels_written_out_by_hand():
    verts, faces = C.hand_triangle()
    view = C.hand_view()
    xs, ys, zw, front = R.project(verts, view)
    assert np.array_equal(xs, [2.5, 6.5, 2.5]) and np.array_equal(ys, [2.5, 2.5, 6.5])  # exact: corners ON pixel centres
    assert np.array_equal(zw, [0.796875, 0.796875, 0.9296875])
    depth = R.depth_buffer(verts, faces, view)
    assert depth.shape == (16, 16) and depth.dtype == np.float32
    got = {(int(i), int(j)) for j, i in zip(*np.nonzero(R.covered(depth)))}
    assert got == C.HAND_TRIANGLE_PIXELS  # centres on the three edges and on the three corners included
    # depth is affine on the screen: 0.796875 on the row y = 2.5, + (0.9296875 - 0.796875) / 4 per row
    for (i, j) in got:
        assert depth[j, i] == np.float32(0.796875 + (j - 2) * 0.033203125)
    # the other winding covers the same pixels with the same depths
    assert np.array_equal(R.depth_buffer(verts, faces[:, ::-1], view), depth)


def test_oracle_shared_edge_leaks_no_pixel_and_agrees_from_both_sides():
    verts, faces = C.shared_edge_pair()
    view = C.hand_view()
    both = R.depth_buffer(verts, faces, view)
    one, two = R.depth_buffer(verts, faces[:1], view), R.depth_buffer(verts, faces[1:], view)
    cov = R.covered(both)
    want = np.zeros((16, 16), bool)
    want[8:13, 8:13] = True
    assert np.array_equal(cov, want)  # every centre of the quad, nothing else
    diag = [(k, k) for k in range(8, 13)]
    for j, i in diag:  # a centre on the shared edge belongs to both triangles, with one depth
        assert R.covered(one)[j, i] and R.covered(two)[j, i] and one[j, i] == two[j, i]
    assert (R.covered(one) & R.covered(two)).sum() == len(diag)
    assert np.array_equal(both, np.minimum(one, two))


def test_oracle_degenerate_triangles_cover_nothing_and_selection_rule():
    verts, faces = C.hand_triangle()
    view = C.hand_view()
    line = np.array([C.at_screen(2.5, 2.5, 8), C.at_screen(4.5, 4.5, 8), C.at_screen(6.5, 6.5, 8)], np.float32)
    assert not R.covered(R.depth_buffer(line, faces, view)).any()                       # zero area, through pixel centres
    assert not R.covered(R.depth_buffer(verts, np.array([[0, 1, 1]], np.int32), view)).any()  # repeated id
    # any-corner rule, order kept, unused points dropped
    v = np.arange(18, dtype=np.float32).reshape(6, 3)
    f = np.array([[0, 1, 2], [2, 3, 4], [3, 4, 5]], np.int32)
    sv, sf = R.select(v, f, [1, 0, 0, 0, 0, 0])
    assert np.array_equal(sf, [[0, 1, 2]]) and np.array_equal(sv, v[:3])
    sv, sf = R.select(v, f, [1, 0, 0, 0, 0, 0], invert=True)
    assert np.array_equal(sf, [[0, 1, 2], [2, 3, 4], [3, 4, 5]]) and np.array_equal(sv, v)
    sv, sf = R.select(v, f, [1, 1, 1, 0, 0, 1], invert=True)
    assert np.array_equal(sv, v[[2, 3, 4, 5]]) and np.array_equal(sf, [[0, 1, 2], [1, 2, 3]])
    assert R.has_non_visible_faces(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)) is False


# ---- the kernels' arithmetic, compiled for the host ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_emu(tmp_path_factory):
    """tests/meshvis_host_emu.cpp: csrc/meshvis_math.h -- the projection, pixel box, edge functions, depth and point test the HIP
    kernels run -- built with the host compiler, contraction off"""
    import ctypes
    import os
    import shutil
    import subprocess

    from invesalius3_amd import polydata_utils as pu
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("meshvis_emu")
    exe = str(tmp / "emu")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(os.path.dirname(__file__), "meshvis_host_emu.cpp")],
                   check=True)

    def run(verts, faces, views):
        v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        cv = pu._c_views(views)
        src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
        with open(src, "wb") as fh:
            fh.write(np.array([len(v), len(f), len(views)], np.int64).tobytes() + v.tobytes() + f.tobytes())
            fh.write(bytes(cv)[: ctypes.sizeof(pu.MeshView) * len(views)])
        subprocess.run([exe, src, dst], check=True)
        raw, off, depths = open(dst, "rb").read(), 0, []
        for view in views:
            w, h = view["size"]
            depths.append(np.frombuffer(raw[off: off + 4 * w * h], np.float32).reshape(h, w))
            off += 4 * w * h
        return depths, np.frombuffer(raw[off:], np.uint8)
    return run


def _emu_cases():
    from invesalius3_amd import polydata_utils as pu
    ball = C.join(C.uv_sphere(10.0, 24, 32, centre=(3.0, -2.0, 40.0)), C.uv_sphere(5.0, 9, 12, centre=(3.0, -2.0, 40.0)))
    sv, sf = C.uv_sphere(10.0, 8, 12)
    n = len(sv)
    degenerate = (np.concatenate([[[40, -35, 5]], sv, [[0, 0, 12], [1, 0, 12], [1, 0, 12]]]).astype(np.float32),
                  np.concatenate([[[n + 1, n + 2, n + 3]], sf + 1, [[n + 1, n + 2, n + 2]]]).astype(np.int32))
    yield "hand triangle", C.hand_triangle(), [C.hand_view()]
    yield "shared edge", C.shared_edge_pair(), [C.hand_view()]
    for bw, bh in ((8, 8), (5, 13), (7, 9)):
        yield "box %d x %d" % (bw, bh), C.box_triangle(3, 5, bw, bh, (128, 128)), [C.hand_view((128, 128))]
    for name, mesh in (("cube", C.cube()), ("nested spheres", ball), ("bowl", C.uv_sphere(10.0, 16, 24, lat_from=0, lat_to=8)),
                       ("degenerate", degenerate)):
        for size in ((800, 800), (64, 64), (48, 96), (96, 48)):
            b = R.bounds_of(mesh[0])
            yield "%s %r" % (name, size), mesh, pu.views_for_positions(b, size=size) + pu.views_for_positions(b, [(1, 1, 1)], size)


def test_kernel_arithmetic_on_the_host_equals_the_restatement(host_emu):
    """every depth bit and every flag, for the hand-built triangles, the boxes at the limit between the two raster kernels, the
    12-triangle cube, two nested spheres, the open bowl and degenerate triangles, square and non-square viewports, axis views and
    (1, 1, 1): the C++ text of the rules and the numpy text of the rules are the same function"""
    for name, (verts, faces), views in _emu_cases():
        depths, flags = host_emu(verts, faces, views)
        want = np.zeros(len(verts), bool)
        for view, got in zip(views, depths):
            ref = R.depth_buffer(verts, faces, view)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), name
            want |= R.visible_in_view(verts, ref, view)
        assert np.array_equal(flags, want.astype(np.uint8)), name
        if name.startswith("nested spheres (800"):
            n_out = len(C.uv_sphere(10.0, 24, 32)[0])
            assert flags[:n_out].all() and not flags[n_out:].any()
