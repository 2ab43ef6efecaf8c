"""Plain-Python statement of the surface import's rules, for tests/test_surface_import_host.py and
tests/test_gpu_surface_import.py: the weld as a dict keyed on the canonical key, the bytes of the files the parsers are tried
on together with the arrays they must return, and the float64 transform.  Nothing here imports the product."""
import struct

import numpy as np

MASK64 = (1 << 64) - 1


# ---- the weld ----------------------------------------------------------------------------------------------------------
def canon(bits: int) -> int:
    """-0.0 is +0.0; every other float32 is its bits"""
    return 0 if bits == 0x80000000 else bits


def keys_of(soup) -> list:
    """the canonical 96-bit key of every corner of the soup, as a tuple of three ints, in corner order"""
    b = np.ascontiguousarray(soup, np.float32).reshape(-1, 3).view(np.uint32)
    return [(canon(int(r[0])), canon(int(r[1])), canon(int(r[2]))) for r in b]


def weld(soup):
    """(verts, faces, counts): ids by first occurrence in corner order, the first occurrence's own bits, facets whose three ids are
    not pairwise different dropped afterwards (their points stay), kept facets in order; ValueError for a non-finite coordinate"""
    s = np.ascontiguousarray(soup, np.float32).reshape(-1, 3)
    if not np.isfinite(s).all():
        raise ValueError("non-finite coordinate")
    ids, first, corner = {}, [], []
    for j, k in enumerate(keys_of(s)):
        i = ids.get(k)
        if i is None:
            i = ids[k] = len(first)
            first.append(j)
        corner.append(i)
    verts = s[np.array(first, np.int64)] if first else np.zeros((0, 3), np.float32)
    tri = np.array(corner, np.int64).reshape(-1, 3)
    keep = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2]) if len(tri) else np.zeros(0, bool)
    faces = tri[keep].astype(np.int32)
    return verts, faces, {"facets_read": len(tri), "vertices": len(verts), "facets": int(keep.sum()), "dropped": int((~keep).sum())}


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the transform -----------------------------------------------------------------------------------------------------
def world_to_inv_affine(affine, spacing, shape, inverse=False):
    a = np.array(affine, np.float64).reshape(4, 4).copy()
    a[1, 3] -= spacing[1] * (shape[1] - 1)
    return np.linalg.inv(a) if inverse else a


def transform(verts, m):
    """float32(((m0 x + m1 y) + m2 z) + m3) per row, every product and sum one rounded float64 operation"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    m = np.asarray(m, np.float64)
    out = np.empty(v.shape, np.float32)
    for r in range(3):
        p0, p1, p2 = m[r, 0] * v[:, 0], m[r, 1] * v[:, 1], m[r, 2] * v[:, 2]
        out[:, r] = (((p0 + p1) + p2) + m[r, 3]).astype(np.float32)
    return out


# ---- files -------------------------------------------------------------------------------------------------------------
def soup_for(ntris: int, seed: int = 0):
    """a reproducible soup with values whose bytes differ in every position (so a wrong byte offset shows)"""
    rng = np.random.default_rng(1000 + seed + ntris)
    return (rng.integers(-(2 ** 30), 2 ** 30, (ntris, 3, 3)).astype(np.float64) / 4099.0).astype(np.float32)


def stl_binary_bytes(soup, header=b"test", attr=0xBEEF) -> bytes:
    """80-byte header, count, 50-byte records with a junk normal and junk attribute bytes (both must be ignored)"""
    s = np.ascontiguousarray(soup, "<f4").reshape(-1, 3, 3)
    out = [header.ljust(80, b"\x01"), struct.pack("<I", len(s))]
    for t in range(len(s)):
        out.append(struct.pack("<3f", 1e30, -2.5, float(t)) + s[t].tobytes() + struct.pack("<H", attr))
    return b"".join(out)


ASCII_STL = (b"solid first\r\n"
             b"  facet normal 0 0 1\r\n    outer loop\r\n"
             b"      vertex 0 0 0\r\n      vertex 1.5e0 0 0\r\n      vertex 0 2.5E-1 0\r\n"
             b"    endloop\r\n  endfacet\r\n"
             b"  facet normal 0 0 1\r\n    outer loop\r\n"
             b"      vertex 1e-3 -0.0 0.1\r\n      vertex 3.4028234e+38 0 0\r\n      vertex 0 16777217 0\r\n"
             b"    endloop\r\n  endfacet\r\n"
             b"endsolid first\r\n"
             b"solid second\r\n"
             b"  facet normal 1 0 0\r\n    outer loop\r\n"
             b"      vertex -1.25E+2 7 8\r\n      vertex 0.30000000000000004 1 2\r\n      vertex 4 5 6e+00\r\n"
             b"    endloop\r\n  endfacet\r\n"
             b"endsolid second\r\n")
# numbers parsed as float64 and rounded once to float32 (16777217 rounds to 16777216; 0.1 to float32's 0.1)
ASCII_STL_SOUP = np.array([[[0, 0, 0], [1.5, 0, 0], [0, 0.25, 0]],
                           [[1e-3, -0.0, 0.1], [3.4028234e+38, 0, 0], [0, 16777217.0, 0]],
                           [[-125.0, 7, 8], [0.30000000000000004, 1, 2], [4, 5, 6]]], np.float64).astype(np.float32)

_PLY_PACK = {"double": "d", "float": "f", "uchar": "B", "int": "i", "short": "h", "ushort": "H"}
PLY_VERTS = np.array([[0.1, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 1.5, 0.25], [-0.5, 0.5, 1e-3], [2, 2, 2]], np.float64)
PLY_POLYS = [[0, 1, 2, 3], [3, 2, 4], [0, 3, 4, 5, 1]]  # a quad, a triangle, a pentagon
# fanned from the first corner
PLY_FACES = np.array([[0, 1, 2], [0, 2, 3], [3, 2, 4], [0, 3, 4], [0, 4, 5], [0, 5, 1]], np.int32)
PLY_EXPECT_VERTS = PLY_VERTS.astype(np.float32)  # x is a double in the file: converted to float32 once


def ply_bytes(fmt: str) -> bytes:
    """x double, y z float, an extra uchar vertex property in the middle, a face property in front of the list"""
    head = ("ply\nformat %s 1.0\ncomment made by the tests\nelement vertex %d\nproperty double x\nproperty uchar red\n"
            "property float y\nproperty float z\nelement face %d\nproperty short flags\nproperty list uchar int vertex_indices\n"
            "end_header\n" % (fmt, len(PLY_VERTS), len(PLY_POLYS))).encode()
    if fmt == "ascii":
        lines = ["%r %d %r %r" % (float(p[0]), 7 + q, float(np.float32(p[1])), float(np.float32(p[2]))) for q, p in enumerate(PLY_VERTS)]
        lines += ["%d %d %s" % (-3 - q, len(poly), " ".join(str(i) for i in poly)) for q, poly in enumerate(PLY_POLYS)]
        return head + ("\n".join(lines) + "\n").encode()
    e = "<" if fmt == "binary_little_endian" else ">"
    body = [struct.pack(e + "dBff", float(p[0]), 7 + q, float(p[1]), float(p[2])) for q, p in enumerate(PLY_VERTS)]
    body += [struct.pack(e + "hB%di" % len(poly), -3 - q, len(poly), *poly) for q, poly in enumerate(PLY_POLYS)]
    return head + b"".join(body)
