"""``invesalius.data.surface`` -- surface import: STL, PLY and VTP files to a welded mesh on the GPU (csrc/k_meshweld.hip,
DESIGN 7q).

``Surface.OnImportSurfaceFile`` -> ``CreateSurfaceFromFile`` -> ``CreateSurfaceFromPolydata`` (surface.py:619-973) read a
surface file through a VTK reader, optionally move it from world to InVesalius coordinates (``ConvertPolydataToInv``,
:850-870), compute normals (feature angle 80, auto-orient) and take volume and area.  Here arrays stand in for
``vtkPolyData`` (``verts`` float32 (N, 3), ``faces`` int32 (T, 3)), the file parsers are host code, and what vtkSTLReader's
point merge does -- one id per coincident corner, first occurrence first -- is a hash insert and two scans on the GPU.

The weld's rules: corners whose float32 coordinates compare equal as numbers are one point (-0.0 == +0.0), the
first occurrence is stored with its own bits, ids go by first occurrence in corner order, facets whose ids are not pairwise
different are dropped afterwards (their points stay), and a coordinate that is not finite is a ValueError.
`surface_process.join_surface_pieces` keeps its own host merge (raw bits, degenerate facets kept).

PARITY UNPINNED: VTK is not installed; the rules are pinned bit for bit against their plain-Python restatement
(tests/_surface_import_ref.py).  OBJ (vtkOBJReader splits points per normal and texture index) and 3MF (lib3mf) stay out."""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L

STL_HEADER, STL_RECORD = 84, 50
MAX_FACETS = L.WELD_MAX_CORNERS // 3
MSG_UNKNOWN_FORMAT = "File format not reconized by InVesalius"      # (the reference's spelling, surface.py:828)
MSG_NOT_ABLE = "InVesalius was not able to import this surface"      # surface.py:841

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


# ---- limits, checked on the host before the library is touched -------------------------------------------------------
def check_facet_count(ntris: int) -> int:
    """3 T <= 2^31 - 1, or ValueError (corner indices are uint32 below the table's empty mark, face ids int32)"""
    if ntris < 0 or 3 * ntris > L.WELD_MAX_CORNERS:
        raise ValueError("a soup of %d triangles has more than 2^31 - 1 corners" % ntris)
    return int(ntris)


def weld_slots(n_corners: int) -> int:
    """slots of the weld's table for this many corners: the power of two >= 2 * corners (ivx_mesh_weld_slots; no device needed)"""
    out = ctypes.c_uint64(0)
    L.check(L.lib().ivx_mesh_weld_slots(ctypes.c_int64(int(n_corners)), ctypes.byref(out)), "mesh_weld_slots")
    return int(out.value)


def counts_dict(words, facets_read: int) -> dict:
    """the weld's count words (IVX_WELD_* of include/ivx.h) as a dict; ValueError / RuntimeError for its two flags"""
    w = [int(x) for x in words]
    if w[L.WELD_OVERRUN]:
        raise RuntimeError("mesh weld: a probe walked the whole table (internal error)")
    if w[L.WELD_NONFINITE]:
        raise ValueError("mesh weld: the soup holds a coordinate that is not finite")
    return {"facets_read": int(facets_read), "vertices": w[L.WELD_VERTS], "facets": w[L.WELD_KEPT], "dropped": w[L.WELD_DROPPED],
            "slots": (1 << w[L.WELD_LOG2_SLOTS]) if facets_read else 0, "max_probe": w[L.WELD_MAX_PROBE],
            "probe_histogram": w[L.WELD_HIST:L.WELD_HIST + 16]}


# ---- STL ---------------------------------------------------------------------------------------------------------------
def stl_kind(data) -> str:
    """``"binary"`` exactly when ``len == 84 + 50 * count`` (the little-endian uint32 at byte 80); otherwise ``"ascii"`` when the
    first non-blank token is ``solid``; otherwise ValueError -- a truncated file or one with trailing bytes is an error."""
    n = len(data)
    if n >= STL_HEADER and n == STL_HEADER + STL_RECORD * int.from_bytes(bytes(data[80:84]), "little"):
        return "binary"
    tokens = bytes(data[:4096]).split(None, 1)
    if tokens and tokens[0] == b"solid":
        return "ascii"
    raise ValueError("not an STL file: %d bytes are neither 84 + 50 * count nor text that starts with 'solid'" % n)


def stl_binary_soup(data) -> np.ndarray:
    """the (T, 3, 3) float32 soup of a binary STL's bytes: 50-byte records from byte 84 -- 12 bytes of normal (ignored), 9
    float32, 2 attribute bytes (ignored)"""
    rec = np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")])
    count = (len(data) - STL_HEADER) // STL_RECORD
    return np.ascontiguousarray(np.frombuffer(data, rec, count=count, offset=STL_HEADER)["v"], dtype=np.float32)


def stl_ascii_soup(data) -> np.ndarray:
    """every ``vertex x y z`` line of every solid of an ASCII STL, three per facet: numbers parsed as float64 and rounded once
    to float32; a facet with other than three vertices is a ValueError"""
    nums, in_facet, nv = [], False, 0
    for ln, raw in enumerate(bytes(data).splitlines(), 1):
        tok = raw.split()
        if not tok:
            continue
        word = tok[0].lower()
        if word == b"facet":
            if in_facet:
                raise ValueError("ascii STL line %d: facet inside a facet" % ln)
            in_facet, nv = True, 0
        elif word == b"vertex":
            if not in_facet or len(tok) != 4:
                raise ValueError("ascii STL line %d: a vertex line is 'vertex x y z' inside a facet" % ln)
            try:
                nums.extend(float(t) for t in tok[1:])
            except ValueError:
                raise ValueError("ascii STL line %d: %r is not a number" % (ln, raw)) from None
            nv += 1
        elif word == b"endfacet":
            if not in_facet or nv != 3:
                raise ValueError("ascii STL line %d: a facet with %d vertices (three are needed)" % (ln, nv))
            in_facet = False
    if in_facet:
        raise ValueError("ascii STL: the last facet is not closed")
    with np.errstate(over="ignore"):
        return np.array(nums, np.float64).astype(np.float32).reshape(-1, 3, 3)


def read_stl(path) -> np.ndarray:
    """The triangle soup of an STL file, (T, 3, 3) float32, binary or ASCII (`stl_kind`).  A host parser: no library call."""
    with open(path, "rb") as f:
        data = f.read()
    soup = stl_binary_soup(data) if stl_kind(data) == "binary" else stl_ascii_soup(data)
    check_facet_count(len(soup))
    return soup


def write_stl_ascii(path, tris, name="ascii"):
    """vtkSTLWriter's ASCII type (surface.py:1831-1833) as far as our own reader is concerned: `read_stl` returns the same
    float32 soup (17 significant digits round-trip a float32 through float64).  VTK's number formatting is not claimed."""
    tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 3, 3)
    v = tris.astype(np.float64)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.divide(n, ln, out=np.zeros_like(n), where=ln > 0)
    with open(path, "w", newline="\n") as f:
        f.write("solid %s\n" % name)
        for t in range(len(tris)):
            f.write(" facet normal %r %r %r\n  outer loop\n" % tuple(float(x) for x in n[t]))
            for c in range(3):
                f.write("   vertex %r %r %r\n" % tuple(float(x) for x in v[t, c]))
            f.write("  endloop\n endfacet\n")
        f.write("endsolid %s\n" % name)


# ---- PLY ---------------------------------------------------------------------------------------------------------------
def _ply_header(data):
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("not a PLY file: no 'ply' ... 'end_header'")
    body = data.find(b"\n", end)
    if body < 0:
        raise ValueError("PLY: the header's last line is not closed")
    fmt, elements = None, []
    for raw in data[:end].splitlines()[1:]:
        tok = raw.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format" and len(tok) >= 2:
            fmt = tok[1]
        elif tok[0] == "element" and len(tok) == 3:
            elements.append({"name": tok[1], "count": int(tok[2]), "props": []})
        elif tok[0] == "property" and elements:
            if tok[1] == "list" and len(tok) == 5:
                kinds = (tok[2], tok[3])
                prop = ("list", tok[4]) + kinds
            elif len(tok) == 3:
                kinds = (tok[1],)
                prop = ("scalar", tok[2], tok[1])
            else:
                raise ValueError("PLY: cannot read the header line %r" % raw)
            for k in kinds:
                if k not in _PLY_TYPES:
                    raise ValueError("PLY: unknown type %r" % k)
            elements[-1]["props"].append(prop)
        else:
            raise ValueError("PLY: cannot read the header line %r" % raw)
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError("PLY: format %r is none of ascii, binary_little_endian, binary_big_endian" % fmt)
    return fmt, elements, body + 1


def _ply_rows_ascii(tokens, pos, el):
    """the rows of one element from the token list: per row a list with one entry per property (a list for a list property)"""
    rows = []
    try:
        for _ in range(el["count"]):
            row = []
            for p in el["props"]:
                if p[0] == "scalar":
                    row.append(float(tokens[pos]))
                    pos += 1
                else:
                    k = int(float(tokens[pos]))
                    row.append([float(t) for t in tokens[pos + 1:pos + 1 + k]])
                    if k < 0 or len(row[-1]) != k:
                        raise IndexError
                    pos += 1 + k
            rows.append(row)
    except (IndexError, ValueError):
        raise ValueError("PLY: element %r is shorter than its header says" % el["name"]) from None
    return rows, pos


def _ply_rows_binary(data, pos, el, order):
    props = el["props"]
    if all(p[0] == "scalar" for p in props):  # one structured read
        dt = np.dtype([("f%d" % q, order + _PLY_TYPES[p[2]]) for q, p in enumerate(props)])
        if pos + dt.itemsize * el["count"] > len(data):
            raise ValueError("PLY: element %r is shorter than its header says" % el["name"])
        a = np.frombuffer(data, dt, count=el["count"], offset=pos)
        return [[a["f%d" % q] for q in range(len(props))]], pos + dt.itemsize * el["count"], True
    lists = [q for q, p in enumerate(props) if p[0] == "list"]
    if len(lists) == 1 and el["count"]:
        # every polygon as long as the first one (the usual all-triangle file): one structured read, kept only if every count agrees
        before = sum(np.dtype(_PLY_TYPES[p[2]]).itemsize for p in props[:lists[0]])
        ct = np.dtype(order + _PLY_TYPES[props[lists[0]][2]])
        if pos + before + ct.itemsize <= len(data):
            k = int(np.frombuffer(data, ct, count=1, offset=pos + before)[0])
            fields = []
            for q, p in enumerate(props):
                if p[0] == "scalar":
                    fields.append(("f%d" % q, order + _PLY_TYPES[p[2]]))
                else:
                    fields += [("c%d" % q, ct), ("f%d" % q, order + _PLY_TYPES[p[3]], (max(k, 0),))]
            dt = np.dtype(fields)
            if k >= 0 and pos + dt.itemsize * el["count"] <= len(data):
                a = np.frombuffer(data, dt, count=el["count"], offset=pos)
                if (a["c%d" % lists[0]] == k).all():
                    return [[a["f%d" % q] for q in range(len(props))]], pos + dt.itemsize * el["count"], True
    rows = []
    try:
        for _ in range(el["count"]):
            row = []
            for p in props:
                if p[0] == "scalar":
                    dt = np.dtype(order + _PLY_TYPES[p[2]])
                    row.append(float(np.frombuffer(data, dt, count=1, offset=pos)[0]))
                    pos += dt.itemsize
                else:
                    ct, it = np.dtype(order + _PLY_TYPES[p[2]]), np.dtype(order + _PLY_TYPES[p[3]])
                    k = int(np.frombuffer(data, ct, count=1, offset=pos)[0])
                    pos += ct.itemsize
                    row.append(np.frombuffer(data, it, count=k, offset=pos).tolist())
                    pos += it.itemsize * k
            rows.append(row)
    except ValueError:
        raise ValueError("PLY: element %r is shorter than its header says" % el["name"]) from None
    return rows, pos, False


def read_ply(path):
    """``(verts (V, 3) float32, faces (T, 3) int32)`` of a PLY file in the ``ascii``, ``binary_little_endian`` or
    ``binary_big_endian`` format.  The vertex properties ``x y z`` may have any PLY scalar type and are converted to float32,
    other vertex properties are skipped; the face list is ``vertex_indices`` or ``vertex_index``, other face properties are
    skipped; a polygon with more than three corners is fanned from its first corner (DEVIATION: vtkTriangleFilter
    ear-clips).  No weld, as with vtkPLYReader.  A host parser: no library call."""
    with open(path, "rb") as f:
        data = f.read()
    fmt, elements, pos = _ply_header(data)
    tokens = data[pos:].split() if fmt == "ascii" else None
    tpos = 0
    order = "<" if fmt == "binary_little_endian" else ">"
    verts, polys = None, []
    for el in elements:
        names = [p[1] for p in el["props"]]
        if fmt == "ascii":
            rows, tpos = _ply_rows_ascii(tokens, tpos, el)
            columns = False
        else:
            rows, pos, columns = _ply_rows_binary(data, pos, el, order)
        if el["name"] == "vertex":
            if not all(c in names for c in "xyz"):
                raise ValueError("PLY: the vertex element has no x, y, z")
            ix = [names.index(c) for c in "xyz"]
            if columns:
                cols = [np.asarray(rows[0][q]) for q in ix]
            else:
                cols = [np.array([r[q] for r in rows], np.float64) for q in ix]
            with np.errstate(over="ignore"):
                verts = np.stack([c.astype(np.float32) for c in cols], axis=1) if el["count"] else np.zeros((0, 3), np.float32)
        elif el["name"] == "face":
            which = [q for q, p in enumerate(el["props"]) if p[0] == "list" and p[1] in ("vertex_indices", "vertex_index")]
            if not which:
                raise ValueError("PLY: the face element has no vertex_indices list")
            polys = np.asarray(rows[0][which[0]]).tolist() if columns else [[int(i) for i in r[which[0]]] for r in rows]
    if verts is None:
        raise ValueError("PLY: no vertex element")
    tris = []
    for poly in polys:
        if len(poly) < 3:
            raise ValueError("PLY: a face with %d corners" % len(poly))
        for q in range(1, len(poly) - 1):
            tris.append((poly[0], poly[q], poly[q + 1]))
    faces = np.array(tris, np.int64).reshape(-1, 3)
    if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError("PLY: face index outside [0, %d)" % len(verts))
    return np.ascontiguousarray(verts), faces.astype(np.int32)


def write_ply_ascii(path, verts, faces):
    """vtkPLYWriter's ASCII type (surface.py:1835-1838) as far as our own reader is concerned: `read_ply` returns the same
    arrays.  VTK's number formatting is not claimed."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    with open(path, "w", newline="\n") as fh:
        fh.write("ply\nformat ascii 1.0\ncomment InVesalius\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
        for p in v.astype(np.float64):
            fh.write("%r %r %r\n" % tuple(float(x) for x in p))
        for t in f:
            fh.write("3 %d %d %d\n" % tuple(int(x) for x in t))


# ---- the weld, the transform, Merge ------------------------------------------------------------------------------------
def weld_soup(tris):
    """``(verts, faces, counts)`` of the soup `tris` ((T, 3, 3) float32) by the rules above, host arrays in and out
    (ivx_mesh_weld).  `counts`: facets read, vertices, facets kept, dropped, the table's slots and its walk-length histogram."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 3, 3)
    nt = check_facet_count(len(t))
    verts, faces = np.empty((3 * nt, 3), np.float32), np.empty((nt, 3), np.int32)
    words = np.zeros(L.WELD_COUNT_WORDS, np.int64)
    L.check(L.lib().ivx_mesh_weld(L.ptr(t), ctypes.c_int64(nt), L.ptr(verts), L.ptr(faces), L.ptr(words)), "mesh_weld")
    c = counts_dict(words, nt)
    verts.resize((c["vertices"], 3), refcheck=False)
    faces.resize((c["facets"], 3), refcheck=False)
    return verts, faces, c


def weld_stl_bytes(data):
    """`weld_soup` of a binary STL's bytes, unpacked on the device (ivx_mesh_stl_weld)"""
    if stl_kind(data) != "binary":
        raise ValueError("not a binary STL")
    nt = check_facet_count((len(data) - STL_HEADER) // STL_RECORD)
    raw = np.frombuffer(data, np.uint8)
    verts, faces = np.empty((3 * nt, 3), np.float32), np.empty((nt, 3), np.int32)
    words = np.zeros(L.WELD_COUNT_WORDS, np.int64)
    L.check(L.lib().ivx_mesh_stl_weld(L.ptr(raw), ctypes.c_size_t(len(raw)), L.ptr(verts), L.ptr(faces), L.ptr(words)), "mesh_stl_weld")
    c = counts_dict(words, nt)
    verts.resize((c["vertices"], 3), refcheck=False)
    faces.resize((c["facets"], 3), refcheck=False)
    return verts, faces, c


def world_to_invesalius_affine(affine, spacing, matrix_shape, inverse=False) -> np.ndarray:
    """``Slice.get_world_to_invesalius_vtk_affine`` (slice_.py:325-359): the 4 x 4 float64 affine with
    ``affine[1, 3] -= spacing[1] * (matrix_shape[1] - 1)``, inverted when `inverse`"""
    a = np.array(affine, np.float64).reshape(4, 4).copy()
    a[1, -1] -= float(spacing[1]) * (int(matrix_shape[1]) - 1)
    if inverse:
        a = np.linalg.inv(a)
    return np.ascontiguousarray(a)


def transform_points(verts, matrix) -> np.ndarray:
    """``float32(((m0 x + m1 y) + m2 z) + m3)`` per row of the 4 x 4 `matrix`, in float64 without contraction (ivx_mesh_transform_points)"""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    m = np.ascontiguousarray(matrix, dtype=np.float64).reshape(4, 4)
    out = np.empty_like(v)
    L.check(L.lib().ivx_mesh_transform_points(L.ptr(v), ctypes.c_int64(len(v)), L.ptr(m), L.ptr(out)), "mesh_transform_points")
    return out


def ConvertPolydataToInv(verts, affine, spacing, matrix_shape, inverse=False) -> np.ndarray:
    """``SurfaceManager.ConvertPolydataToInv`` (surface.py:850-870) on a point array: world / scanner coordinates to
    InVesalius coordinates (with the shift in y), or back with `inverse`"""
    return transform_points(verts, world_to_invesalius_affine(affine, spacing, matrix_shape, inverse))


def Merge(meshes):
    """``pu.Merge`` (vtkAppendPolyData, used by ``_export_surface`` when several surfaces are shown): the ``(verts, faces)``
    pairs appended in order, every mesh's ids offset by the points before it"""
    vs, fs, base = [], [], 0
    for verts, faces in meshes:
        v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        if len(f) and (f.min() < 0 or f.max() >= len(v)):
            raise ValueError("Merge: face index outside [0, %d)" % len(v))
        vs.append(v)
        fs.append(f.astype(np.int64) + base)
        base += len(v)
    if not vs:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    if base > 2 ** 31 - 1:
        raise ValueError("Merge: more than 2^31 - 1 points")
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


# ---- CreateSurfaceFromFile ---------------------------------------------------------------------------------------------
@dataclass
class ImportedSurface:
    """What `CreateSurfaceFromFile` returns: the mesh resident on the GPU (``surface.polydata``), the display copy
    vtkPolyDataNormals makes for the actor (points split at sharp edges, their normals), the measures and the weld's counts"""
    mesh: object
    normals: np.ndarray
    normal_verts: np.ndarray
    normal_faces: np.ndarray
    volume: float
    area: float
    name: str
    format: str
    counts: dict = field(default_factory=dict)

    def close(self):
        self.mesh.close()


def CreateSurfaceFromFile(path, weld=None, convert_to_inv=None, stream=None) -> ImportedSurface:
    """``SurfaceManager.CreateSurfaceFromFile`` + ``CreateSurfaceFromPolydata`` (surface.py:625-973) for ``.stl``, ``.ply``
    and ``.vtp`` (the extension decides, case-insensitive).  `weld`: None = STL yes (vtkSTLReader merges), PLY and VTP no;
    True forces a weld of ``verts[faces]``.  `convert_to_inv`: None, or ``(affine, spacing, matrix_shape)`` for
    `ConvertPolydataToInv`, done on the resident points.  Then normals (feature angle 80, auto-orient:
    `surface_process.point_normals`) and volume and area (`surface_process.mass_properties`).
    ValueError: an unknown extension (the reference's message), a file without points ("not able to import"), a malformed
    file, a coordinate that is not finite."""
    from . import polydata_utils as pu
    from . import surface_process as sp

    ext = os.path.splitext(str(path))[1].lower()
    if ext not in (".stl", ".ply", ".vtp"):
        raise ValueError(MSG_UNKNOWN_FORMAT)
    name = os.path.splitext(os.path.split(str(path))[-1])[0]
    counts = {}
    if ext == ".stl":
        with open(path, "rb") as f:
            data = f.read()
        kind = stl_kind(data)
        fmt = "stl-" + kind
        nt = check_facet_count((len(data) - STL_HEADER) // STL_RECORD) if kind == "binary" else None
        if nt == 0:
            raise ValueError(MSG_NOT_ABLE)
        if kind == "binary" and weld is not False:
            mesh = pu.DeviceMesh.from_stl_bytes(data, stream)
        else:
            soup = stl_binary_soup(data) if kind == "binary" else stl_ascii_soup(data)
            if not len(soup):
                raise ValueError(MSG_NOT_ABLE)
            check_facet_count(len(soup))
            mesh = (pu.DeviceMesh.from_soup(soup, stream) if weld is not False else
                    pu.DeviceMesh.upload(soup.reshape(-1, 3), np.arange(3 * len(soup), dtype=np.int32).reshape(-1, 3), stream))
        counts = getattr(mesh, "weld_counts", None) or {"facets_read": mesh.ntris, "vertices": mesh.nverts, "facets": mesh.ntris, "dropped": 0}
    else:
        verts, faces = read_ply(path) if ext == ".ply" else sp.read_vtp(path)
        fmt = ext[1:]
        if not len(verts):
            raise ValueError(MSG_NOT_ABLE)
        if weld:
            if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
                raise ValueError("%s: face index outside [0, %d)" % (path, len(verts)))
            mesh = pu.DeviceMesh.from_soup(verts[faces], stream)
            counts = mesh.weld_counts
        else:
            mesh = pu.DeviceMesh.upload(verts, faces, stream)
            counts = {"facets_read": len(faces), "vertices": len(verts), "facets": len(faces), "dropped": 0}
    try:
        if mesh.nverts == 0:
            raise ValueError(MSG_NOT_ABLE)
        if convert_to_inv:
            affine, spacing, shape = convert_to_inv
            m = world_to_invesalius_affine(affine, spacing, shape)
            L.check(L.lib().ivx_dev_mesh_transform_points(mesh.verts.ptr, ctypes.c_int64(mesh.nverts), L.ptr(m), mesh.verts.ptr, mesh.stream),
                    "mesh_transform_points")
        v, f = mesh.download()
        nv, nf, pn, _ = sp.point_normals(v, f, feature_angle=80.0, splitting=True, auto_orient=True)
        volume, area = sp.mass_properties(v, f)
    except Exception:
        mesh.close()
        raise
    return ImportedSurface(mesh, pn, nv, nf, float(volume), float(area), name, fmt, dict(counts))
