"""Inputs of the surface view's tests: small meshes, cameras and scenes, shared by the CPU tests (the restatement
against the host build of csrc/surfview_math.h) and the GPU tests.  Every mesh has at most ~5 000 triangles and every picture
at most 96 x 96 pixels, except the cube at 256 x 256 and the 257 x 3 viewport.

A scene is a dict: name, layers (tests/_surface_view_ref.layer), cam, ties (True when two triangles may have the same depth at
one pixel centre: such a scene is left out of the shuffled-launch-order test)."""
import numpy as np

import _surface_view_ref as R

VIEW_NAMES = ("front", "back", "right", "left", "top", "bottom", "iso")


# ---- cameras ---------------------------------------------------------------------------------------------------------------------
def hand_cam(size=(16, 16)):
    """looks down -z with one world unit per pixel: X = x + W / 2, Y = H / 2 - y, t = -z, all exact for small half-integers"""
    W, H = size
    return {"focal": (0.0, 0.0, 0.0), "right": (1.0, 0.0, 0.0), "up": (0.0, 1.0, 0.0), "dir": (0.0, 0.0, -1.0),
            "parallel_scale": H / 2.0, "viewport": (int(W), int(H))}


def at_screen(X, Y, t, size=(16, 16)):
    """the world point that hand_cam(size) puts at screen (X, Y) with depth t"""
    W, H = size
    return (X - W / 2.0, H / 2.0 - Y, -t)


def bounds_of(*meshes):
    v = np.concatenate([np.asarray(m, np.float32).reshape(-1, 3) for m in meshes])
    lo, hi = v.min(0), v.max(0)
    return (float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1]), float(lo[2]), float(hi[2]))


def view_cam(view, bounds, size):
    from invesalius3_amd import surface_view
    return surface_view.camera_for_bounds(view, bounds, size)


# ---- meshes ----------------------------------------------------------------------------------------------------------------------
def hand_triangle(size=(16, 16), t=(3.0, 3.0, 3.0)):
    """corners ON the pixel centres (2.5, 2.5), (2.5, 6.5), (6.5, 2.5), walked so that it faces the viewer"""
    verts = np.array([at_screen(2.5, 2.5, t[0], size), at_screen(2.5, 6.5, t[1], size), at_screen(6.5, 2.5, t[2], size)], np.float32)
    return verts, np.array([[0, 1, 2]], np.int32)


HAND_TRIANGLE_PIXELS = {(i, j) for i in range(2, 7) for j in range(2, 7) if i + j <= 8}  # edges and corners included


def shared_edge_pair(size=(16, 16)):
    """the square of centres 8.5 .. 12.5 split along its diagonal, whose five centres lie on the shared edge"""
    verts = np.array([at_screen(8.5, 8.5, 2.0, size), at_screen(12.5, 8.5, 2.0, size), at_screen(12.5, 12.5, 2.0, size),
                      at_screen(8.5, 12.5, 2.0, size)], np.float32)
    return verts, np.array([[0, 2, 1], [0, 3, 2]], np.int32)


def box_triangle(x0, y0, bw, bh, size, t=5.0):
    """a front-facing right triangle whose pixel box is exactly bw x bh with its corner at pixel (x0, y0)"""
    xa, ya = x0 + 0.5, y0 + 0.5
    xb = x0 + bw - 0.5 if bw > 1 else xa + 0.4375
    yb = y0 + bh - 0.5 if bh > 1 else ya + 0.4375
    verts = np.array([at_screen(xa, ya, t, size), at_screen(xa, yb, t, size), at_screen(xb, ya, t, size)], np.float32)
    return verts, np.array([[0, 1, 2]], np.int32)


def cube(half=10.0, centre=(0.0, 0.0, 0.0)):
    """twelve triangles, outward"""
    c = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64) * half + np.asarray(centre)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    faces = [t for a, b, c_, d in quads for t in ((a, b, c_), (a, c_, d))]
    return _outward(c.astype(np.float32), np.array(faces, np.int32))


def _outward(verts, faces):
    v = verts.astype(np.float64)
    vol = np.einsum("ij,ij->i", v[faces[:, 0]] - v.mean(0), np.cross(v[faces[:, 1]] - v.mean(0), v[faces[:, 2]] - v.mean(0))).sum()
    assert vol != 0
    return verts, (faces if vol > 0 else np.ascontiguousarray(faces[:, ::-1]))


def icosphere(radius=10.0, level=3, centre=(0.0, 0.0, 0.0)):
    """20 * 4^level outward triangles (level 3: 1 280, 642 points); returns verts, faces and the unit normals = positions"""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    unit = np.array(v, np.float64)
    verts, faces = _outward((unit * radius).astype(np.float32), np.array(f, np.int32))
    normals = unit.astype(np.float32)
    return (verts + np.asarray(centre, np.float32)).astype(np.float32), faces, normals


def tilted_sheet(size=(32, 32)):
    """a front-facing quad of two triangles whose depth runs from -6 to +6 across the picture: t crosses zero"""
    verts = np.array([at_screen(4.25, 5.5, -6.0, size), at_screen(27.75, 5.5, 6.0, size), at_screen(27.75, 26.25, 6.0, size),
                      at_screen(4.25, 26.25, -6.0, size)], np.float32)
    return verts, np.array([[0, 2, 1], [0, 3, 2]], np.int32)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def _scene(name, layers, cam, ties=False):
    return {"name": name, "layers": layers, "cam": cam, "ties": ties}


def scenes():
    """every case of the list, the nine-surface error apart (nine_layers)"""
    out = []
    L = R.layer
    green, red, blue = (0.33, 1.0, 0.33), (1.0, 0.33, 0.33), (0.25, 0.5, 1.0)
    # the hand-built triangles
    out.append(_scene("hand triangle", [L(*hand_triangle(), colour=green)], hand_cam()))
    out.append(_scene("hand triangle tilted", [L(*hand_triangle(t=(3.0, 1.0, 7.0)), colour=green)], hand_cam()))
    out.append(_scene("shared edge", [L(*shared_edge_pair(), colour=red)], hand_cam(), ties=True))
    v, f = hand_triangle()
    out.append(_scene("coincident", [L(v, np.concatenate([f, f]), colour=red)], hand_cam(), ties=True))
    out.append(_scene("coincident copies", [L(np.concatenate([v, v]), np.concatenate([f + 3, f]), colour=red)], hand_cam(), ties=True))
    out.append(_scene("reversed winding", [L(v, f[:, ::-1], colour=red)], hand_cam()))
    # the pixel box at the limit between the two raster kernels
    for bw, bh in ((8, 8), (5, 13), (13, 5), (64, 1), (65, 1), (1, 65)):
        out.append(_scene("box %d x %d" % (bw, bh), [L(*box_triangle(3, 5, bw, bh, (96, 96)), colour=blue)], hand_cam((96, 96))))
    # the cube: all big
    cv, cf = cube()
    out.append(_scene("cube 256", [L(cv, cf, colour=green)], view_cam("iso", bounds_of(cv), (256, 256))))
    # the icosphere with its analytic normals, from all seven views
    sv, sf, sn = icosphere()
    for view in VIEW_NAMES:
        out.append(_scene("icosphere %s" % view, [L(sv, sf, sn, colour=green)], view_cam(view, bounds_of(sv), (96, 96))))
    out.append(_scene("icosphere without normals", [L(sv, sf, None, colour=green)], view_cam("iso", bounds_of(sv), (64, 64))))
    # depth crossing zero
    out.append(_scene("tilted sheet", [L(*tilted_sheet(), colour=blue)], hand_cam((32, 32))))
    # partly and wholly outside the viewport
    b = bounds_of(sv)
    pv, pf, pn = icosphere(centre=(9.0, -14.0, 3.0))
    out.append(_scene("partly outside", [L(pv, pf, pn, colour=red)], view_cam("front", b, (64, 64))))
    ov, of_, on = icosphere(level=1, centre=(300.0, 0.0, 0.0))
    out.append(_scene("wholly outside", [L(ov, of_, on, colour=red)], view_cam("front", b, (64, 64))))
    # degenerate triangles among good ones: zero area, repeated ids, a corner that is not finite
    s1v, s1f, s1n = icosphere(level=1)
    n = len(s1v)
    dv = np.concatenate([s1v, [[0, 0, 30], [1, 0, 30], [2, 0, 30], [np.inf, 0, 0], [np.nan, 1, 1]]]).astype(np.float32)
    dn = np.concatenate([s1n, np.zeros((5, 3), np.float32)])
    df = np.concatenate([[[n, n + 1, n + 2]], s1f[:40], [[n, n + 1, n + 1], [0, 1, n + 3], [n + 4, 2, 3]], s1f[40:], [[5, 5, 5]]]).astype(np.int32)
    out.append(_scene("degenerate", [L(dv, df, dn, colour=green)], view_cam("iso", bounds_of(s1v), (48, 48))))
    out.append(_scene("empty mesh", [L(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))], hand_cam()))
    out.append(_scene("no surface", [], hand_cam()))
    # nested spheres
    iv, if_, in_ = icosphere(radius=5.0, level=2)
    uv, uf, un = icosphere(radius=10.0, level=2)
    for view in ("iso", "top"):
        cam = view_cam(view, bounds_of(uv), (64, 64))
        out.append(_scene("opaque inside translucent %s" % view, [L(uv, uf, un, colour=green, transparency=0.6), L(iv, if_, in_, colour=red)], cam))
        out.append(_scene("translucent inside opaque %s" % view, [L(iv, if_, in_, colour=red, transparency=0.5), L(uv, uf, un, colour=green)], cam))
    cam = view_cam("iso", bounds_of(uv), (64, 64))
    out.append(_scene("two translucent", [L(iv, if_, in_, colour=red, transparency=0.5), L(uv, uf, un, colour=green, transparency=0.25)], cam))
    # two identical meshes in different colours: the lower surface index is in front
    out.append(_scene("identical meshes", [L(uv, uf, un, colour=red, transparency=0.5), L(uv, uf, un, colour=blue)], cam))
    out.append(_scene("identical meshes reversed", [L(uv, uf, un, colour=blue), L(uv, uf, un, colour=red, transparency=0.5)], cam))
    # eight surfaces
    out.append(_scene("eight surfaces", eight_layers(), view_cam("iso", (-12.0, 12.0, -12.0, 12.0, -12.0, 12.0), (64, 64))))
    # viewports
    for size in ((1, 1), (257, 3), (48, 96), (96, 48)):
        out.append(_scene("viewport %d x %d" % size, [L(uv, uf, un, colour=green), L(iv + np.float32(6.0), if_, in_, colour=red, transparency=0.3)],
                          view_cam("iso", bounds_of(uv), size)))
    return out


def eight_layers(count=8):
    """`count` small spheres along a diagonal, alternately opaque and translucent, in `count` colours"""
    from invesalius3_amd import surface_view
    layers = []
    for k in range(count):
        v, f, nrm = icosphere(radius=4.0, level=1, centre=(-8.0 + 2.0 * k, 6.0 - 1.5 * k, -7.0 + 2.0 * k))
        layers.append(R.layer(v, f, nrm, colour=surface_view.SURFACE_COLOUR[k], transparency=(0.0, 0.4, 0.7)[k % 3]))
    return layers
