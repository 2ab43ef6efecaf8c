"""Inputs shared by the surface visibility tests (CPU and GPU): a hand-made view whose projection is exact in binary, the
hand-built triangles, and small analytic meshes.  No product code here."""
import numpy as np


def hand_view(size=(16, 16)):
    """eye at the origin looking along +z, tan(half angle) = 1: a point (x, y, z) lands on xs = (x / z + 1) * W / 2, and with
    near 2, far 34 and z a power of two, zw = 34 (z - 2) / (32 z) is exact too."""
    return {"eye": [0.0, 0.0, 0.0], "right": [1.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "fwd": [0.0, 0.0, 1.0], "near": 2.0, "far": 34.0,
            "tan_half": 1.0, "aspect": size[0] / size[1], "size": (int(size[0]), int(size[1]))}


def at_screen(xs, ys, z, size=(16, 16)):
    """the world point that `hand_view(size)` projects to (xs, ys) at eye depth z (exact for dyadic xs, ys and z = 2^k; square
    viewports)"""
    assert size[0] == size[1]
    return [(xs / (size[0] / 2) - 1.0) * z, (ys / (size[1] / 2) - 1.0) * z, float(z)]


def hand_triangle():
    """legs on the pixel-centre lines x = 2.5 and y = 2.5, hypotenuse x + y = 9 through the centres (3.5, 5.5) .. (5.5, 3.5);
    the three corners sit on pixel centres; the third corner is twice as deep as the others"""
    verts = np.array([at_screen(2.5, 2.5, 8), at_screen(6.5, 2.5, 8), at_screen(2.5, 6.5, 16)], np.float32)
    return verts, np.array([[0, 1, 2]], np.int32)


HAND_TRIANGLE_PIXELS = {(2, 2), (3, 2), (4, 2), (5, 2), (6, 2),
                        (2, 3), (3, 3), (4, 3), (5, 3),
                        (2, 4), (3, 4), (4, 4),
                        (2, 5), (3, 5),
                        (2, 6)}  # (i, j): column, row


def shared_edge_pair():
    """the square (8.5, 8.5) .. (12.5, 12.5) cut along the diagonal that passes through five pixel centres; corners at eye
    depths 8, 16, 8, 4"""
    verts = np.array([at_screen(8.5, 8.5, 8), at_screen(12.5, 8.5, 16), at_screen(12.5, 12.5, 8), at_screen(8.5, 12.5, 4)], np.float32)
    return verts, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def box_triangle(x0, y0, bw, bh, size):
    """a triangle whose clamped pixel box is exactly bw x bh pixels from (x0, y0), corners at eye depths 8, 16, 8"""
    verts = np.array([at_screen(x0 + 0.25, y0 + 0.25, 8, size), at_screen(x0 + bw - 0.25, y0 + 0.25, 16, size),
                      at_screen(x0 + 0.25, y0 + bh - 0.25, 8, size)], np.float32)
    return verts, np.array([[0, 1, 2]], np.int32)


def cube(lo=(-1.0, -2.0, 3.0), side=4.0):
    c = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32) * np.float32(side) + np.array(lo, np.float32)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c_, d in q for t in ((a, b, c_), (a, c_, d))]
    return c, np.array(f, np.int32)


def uv_sphere(radius, n_lat=12, n_lon=16, centre=(0.0, 0.0, 0.0), lat_from=0, lat_to=None):
    """closed UV sphere (or, with lat_from / lat_to, the band of latitude rows between them: an open bowl); outward winding"""
    lat_to = n_lat if lat_to is None else lat_to
    pts, index = [], {}

    def vid(i, j):
        j %= n_lon
        key = (0, 0) if i == 0 else (n_lat, 0) if i == n_lat else (i, j)
        if key not in index:
            th, ph = np.pi * key[0] / n_lat, 2 * np.pi * key[1] / n_lon
            index[key] = len(pts)
            pts.append([radius * np.sin(th) * np.cos(ph) + centre[0], radius * np.sin(th) * np.sin(ph) + centre[1],
                        radius * np.cos(th) + centre[2]])
        return index[key]

    faces = []
    for i in range(lat_from, lat_to):
        for j in range(n_lon):
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
            if i != 0:
                faces.append((a, b, d))
            if i + 1 != n_lat:
                faces.append((b, c, d))
    return np.array(pts, np.float32), np.array(faces, np.int32)


def join(*meshes):
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + off)
        off += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def shell_mask(n, r_out, r_in):
    """n^3 uint8 mask: a ball of radius r_out with a concentric cavity of radius r_in"""
    c = (n - 1) / 2.0
    z, y, x = np.mgrid[:n, :n, :n]
    d2 = (z - c) ** 2 + (y - c) ** 2 + (x - c) ** 2
    return np.where((d2 <= r_out * r_out) & (d2 > r_in * r_in), 255, 0).astype(np.uint8)
