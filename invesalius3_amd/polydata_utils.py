"""``invesalius.data.polydata_utils`` -- the surface visibility tools on the GPU (csrc/k_meshvis.hip).

``RemoveNonVisibleFaces`` (polydata_utils.py:363-455) and ``HasNonVisibleFaces`` (:281-360) render the surface off screen
from six sides and ask vtkSelectVisiblePoints which points the z-buffer lets through.  Here the renders are a depth-only
software rasteriser in HIP, and arrays stand in for ``vtkPolyData``: ``verts`` float32 (N, 3), ``faces`` int32 (T, 3).
The cameras are built here, on the host, in float64 and handed to the kernels as plain numbers.  `DeviceMesh` is the
same mesh resident in HBM (what ``DeviceVolume.marching_cubes_indexed(download=False)`` leaves behind): with it
threshold -> mesh -> keep largest -> remove non-visible never leaves the device.

The surface connectivity tools (polydata_utils.py:206-278; csrc/k_meshparts.hip) are here as well:
``SplitDisconectedParts``, ``JoinSeedsParts`` and ``SelectLargestPart``, on arrays or on a `DeviceMesh`; `MeshParts` is the
split resident in HBM, every part a view into two grouped buffers.

`DeviceMesh.graph`, `geodesic_distances` and `geodesic` are the device side of the geodesic measure (`measures.py`;
csrc/k_meshgeo.hip): the mesh graph built once per mesh, edge distances pinned to scipy's Dijkstra bit for bit.

PARITY UNPINNED: VTK and its OpenGL rasteriser are not installed; the rules of DESIGN 7f / 7h are pinned bit for bit against
their numpy restatements (tests/_meshvis_ref.py, tests/_mesh_regions_ref.py).  vtkCleanPolyData's merge of coincident points
is not done."""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib as L

POSITIONS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))  # the reference's six, in its order
SIZE = (800, 800)                                                                  # render_window.SetSize(800, 800)
VIEW_ANGLE = 30.0                                                                  # vtkCamera's default


class MeshView(ctypes.Structure):
    """struct ivx_mesh_view (include/ivx.h)."""
    _fields_ = [("eye", ctypes.c_double * 3), ("right", ctypes.c_double * 3), ("up", ctypes.c_double * 3),
                ("fwd", ctypes.c_double * 3), ("znear", ctypes.c_double), ("zfar", ctypes.c_double),
                ("tan_half", ctypes.c_double), ("aspect", ctypes.c_double), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _unit(a):
    ln = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    return [a[0] / ln, a[1] / ln, a[2] / ln]


def views_for_positions(bounds, positions=POSITIONS, size=SIZE) -> list:
    """The cameras of the tool for a mesh with these bounds ``(xmin, xmax, ymin, ymax, zmin, zmax)``: per position the eye at
    ``centre + unit(position) * dist``, looking at the centre, with ``dist = radius / sin(15 deg)`` (ResetCamera, as
    `volume.camera_for_view`), a perspective of 30 degrees, the view up carried along the list the way vtkCamera carries it
    (turned when it gets parallel to the view direction) and ResetCameraClippingRange's near / far from the bounds' corners.
    Each view is a dict of floats: eye, right, up, fwd, near, far, tan_half, aspect, size (+ view_up, dist, centre)."""
    w_px, h_px = int(size[0]), int(size[1])
    if w_px <= 0 or h_px <= 0:
        raise ValueError("size %r must be positive" % (size,))
    b = [float(x) for x in bounds]
    c = [(b[0] + b[1]) / 2, (b[2] + b[3]) / 2, (b[4] + b[5]) / 2]
    w = [b[1] - b[0], b[3] - b[2], b[5] - b[4]]
    radius = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) * 0.5
    if radius == 0.0:
        radius = 1.0
    half = math.radians(VIEW_ANGLE) * 0.5
    dist = radius / math.sin(half)
    up = [0.0, 1.0, 0.0]
    out = []
    for p in positions:
        n = _unit([float(x) for x in p])
        eye = [c[0] + n[0] * dist, c[1] + n[1] * dist, c[2] + n[2] * dist]
        if abs(up[0] * n[0] + up[1] * n[1] + up[2] * n[2]) > 0.999:
            up = [-up[2], up[0], up[1]]  # (and it stays turned for the views that follow)
        fwd = [-n[0], -n[1], -n[2]]
        right = _unit(_cross(fwd, up))
        upv = _cross(right, fwd)
        n0, f0 = math.inf, -math.inf
        for x in (b[0], b[1]):
            for y in (b[2], b[3]):
                for z in (b[4], b[5]):
                    d = ((x - eye[0]) * fwd[0] + (y - eye[1]) * fwd[1]) + (z - eye[2]) * fwd[2]
                    n0, f0 = min(n0, d), max(f0, d)
        near = 0.99 * n0 - 0.5 * (f0 - n0)
        far = 1.01 * f0 + 0.5 * (f0 - near)
        if near >= far:
            near = 0.01 * far
        near = max(near, 0.001 * far)
        out.append({"eye": eye, "right": right, "up": upv, "fwd": fwd, "near": near, "far": far, "tan_half": math.tan(half),
                    "aspect": w_px / h_px, "size": (w_px, h_px), "view_up": list(up), "dist": dist, "centre": c})
    return out


def _c_views(views):
    arr = (MeshView * max(len(views), 1))()
    for q, v in enumerate(views):
        m = arr[q]
        m.eye[:], m.right[:], m.up[:], m.fwd[:] = v["eye"], v["right"], v["up"], v["fwd"]
        m.znear, m.zfar, m.tan_half, m.aspect = v["near"], v["far"], v["tan_half"], v["aspect"]
        m.width, m.height = v["size"]
    return arr


def _mesh(verts, faces):
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    return v, f


class DeviceMesh:
    """An indexed mesh resident on the GPU: two `DeviceBuffer`s, the counts and the stream its kernels run on."""

    def __init__(self, verts_buf, nverts: int, faces_buf, ntris: int, stream=None, owns: bool = False):
        self.verts, self.nverts, self.faces, self.ntris, self.stream, self._owns = verts_buf, int(nverts), faces_buf, int(ntris), stream, owns
        self._graph = None  # the mesh graph of the geodesic measure, built on first use

    @classmethod
    def from_volume(cls, vol, counts=None):
        """The mesh ``vol.marching_cubes_indexed(download=False)`` made; `counts` is what that call returned."""
        nv, nt = counts if counts is not None else vol.marching_cubes_indexed()
        return cls(vol._verts, nv, vol._faces, nt, vol.stream)

    @classmethod
    def upload(cls, verts, faces, stream=None):
        from .device import DeviceBuffer
        v, f = _mesh(verts, faces)
        if len(f) and (f.min() < 0 or f.max() >= len(v)):
            raise ValueError("mesh: face index outside [0, %d)" % len(v))
        m = cls(DeviceBuffer(v.nbytes + 16), len(v), DeviceBuffer(f.nbytes + 16), len(f), stream, owns=True)
        if len(v):
            m.verts.upload(v)
        if len(f):
            m.faces.upload(f)
        return m

    # ---- surface import ----
    @classmethod
    def _weld(cls, soup_buf, ntris: int, stream=None):
        """the weld of the (3 T, 3) float32 soup in `soup_buf` (csrc/k_meshweld.hip): the mesh, its `weld_counts` set; waits
        for the counts, so the caller may free the soup afterwards.  The buffers keep their worst-case room (3 T points)."""
        from . import surface as S
        from .device import DeviceBuffer
        lib = L.lib()
        nb = ctypes.c_size_t(0)
        L.check(lib.ivx_mesh_weld_bytes(ctypes.c_int64(ntris), ctypes.byref(nb)), "mesh_weld_bytes")
        bufs = [DeviceBuffer(nb.value + 16), DeviceBuffer(L.WELD_COUNT_WORDS * 4), DeviceBuffer(ntris * 36 + 16), DeviceBuffer(ntris * 12 + 16)]
        scratch, cnt, ov, of = bufs
        try:
            L.check(lib.ivx_dev_mesh_weld(soup_buf.ptr, ctypes.c_int64(ntris), scratch.ptr, ov.ptr, of.ptr, cnt.ptr, stream), "mesh_weld")
            L.check(lib.ivx_stream_synchronize(stream) if stream else lib.ivx_device_synchronize())
            counts = S.counts_dict(cnt.download((L.WELD_COUNT_WORDS,), np.uint32), ntris)
        except Exception:
            for b in bufs:
                b.close()
            raise
        scratch.close()
        cnt.close()
        m = cls(ov, counts["vertices"], of, counts["facets"], stream, owns=True)
        m.weld_counts = counts
        return m

    @classmethod
    def from_soup(cls, tris, stream=None):
        """The welded mesh of a triangle soup ((T, 3, 3) float32, what an STL file holds): coincident corners share one id, by
        first occurrence; degenerate facets are dropped; a coordinate that is not finite is a ValueError.  `weld_counts`
        holds the counts (`surface.counts_dict`)."""
        from . import surface as S
        from .device import DeviceBuffer
        t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 3, 3)
        S.check_facet_count(len(t))  # (raises before anything is launched)
        soup = DeviceBuffer(t.nbytes + 16)
        try:
            if len(t):
                soup.upload(t)
            return cls._weld(soup, len(t), stream)
        finally:
            soup.close()

    @classmethod
    def from_stl_bytes(cls, data, stream=None):
        """`from_soup` of a binary STL file's bytes: the file goes to the device as it is and is unpacked there"""
        from . import surface as S
        from .device import DeviceBuffer
        if S.stl_kind(data) != "binary":
            raise ValueError("from_stl_bytes takes a binary STL (surface.read_stl parses the ASCII form)")
        nt = S.check_facet_count((len(data) - S.STL_HEADER) // S.STL_RECORD)
        raw = np.frombuffer(data, np.uint8)
        lib = L.lib()
        file_buf, soup, flag = DeviceBuffer(len(raw) + 16), DeviceBuffer(nt * 36 + 16), DeviceBuffer(16)
        try:
            file_buf.upload(raw)
            flag.zero(stream)
            L.check(lib.ivx_dev_stl_unpack(file_buf.ptr, ctypes.c_int64(nt), soup.ptr, flag.ptr, stream), "stl_unpack")
            return cls._weld(soup, nt, stream)  # (the weld raises the non-finite flag for the same coordinates)
        finally:
            for b in (file_buf, soup, flag):
                b.close()

    def sync(self):
        L.check(L.lib().ivx_stream_synchronize(self.stream) if self.stream else L.lib().ivx_device_synchronize())

    def download(self):
        self.sync()
        return self.verts.download((self.nverts, 3), np.float32), self.faces.download((self.ntris, 3), np.int32)

    def bounds(self):
        from .device import DeviceBuffer
        out = DeviceBuffer(64)
        try:
            L.check(L.lib().ivx_dev_mesh_bounds(self.verts.ptr, ctypes.c_int64(self.nverts), out.ptr, self.stream), "mesh_bounds")
            self.sync()  # (the stream does not block the copy below)
            return tuple(float(x) for x in out.download((6,), np.float32))
        finally:
            out.close()

    def visible_flags(self, views):
        """device buffer of one uint8 per point (the caller closes it)"""
        from .device import DeviceBuffer
        flags = DeviceBuffer(self.nverts + 16)
        L.check(L.lib().ivx_dev_mesh_visible_points(self.verts.ptr, ctypes.c_int64(self.nverts), self.faces.ptr, ctypes.c_int64(self.ntris),
                                                    _c_views(views), len(views), flags.ptr, self.stream), "mesh_visible_points")
        return flags

    def select(self, flags, invert: bool = False) -> "DeviceMesh":
        from .device import DeviceBuffer
        ov, of = DeviceBuffer(self.nverts * 12 + 16), DeviceBuffer(self.ntris * 12 + 16)
        nv, nt = ctypes.c_int64(0), ctypes.c_int64(0)
        L.check(L.lib().ivx_dev_mesh_select_points(self.verts.ptr, ctypes.c_int64(self.nverts), self.faces.ptr, ctypes.c_int64(self.ntris),
                                                   flags.ptr, int(bool(invert)), ov.ptr, ctypes.c_int64(self.nverts), of.ptr,
                                                   ctypes.c_int64(self.ntris), ctypes.byref(nv), ctypes.byref(nt), self.stream),
                "mesh_select_points")
        return DeviceMesh(ov, nv.value, of, nt.value, self.stream, owns=True)

    # ---- surface connectivity ----
    def region_labels(self):
        """``(tri_labels int32 (T,), n_regions)``: region r is the r-th region in the order of its first triangle"""
        from .device import DeviceBuffer
        lab = DeviceBuffer(self.ntris * 4 + 16)
        nr = ctypes.c_int64(0)
        try:
            L.check(L.lib().ivx_dev_mesh_region_labels(ctypes.c_int64(self.nverts), self.faces.ptr, ctypes.c_int64(self.ntris), lab.ptr,
                                                       None, ctypes.byref(nr), None, self.stream), "mesh_region_labels")
            self.sync()
            return lab.download((self.ntris,), np.int32), nr.value
        finally:
            lab.close()

    def keep_largest(self) -> "DeviceMesh":
        from .device import DeviceBuffer
        ov, of = DeviceBuffer(self.nverts * 12 + 16), DeviceBuffer(self.ntris * 12 + 16)
        nv, nt = ctypes.c_int64(0), ctypes.c_int64(0)
        L.check(L.lib().ivx_dev_mesh_keep_largest(self.verts.ptr, ctypes.c_int64(self.nverts), self.faces.ptr, ctypes.c_int64(self.ntris),
                                                  ov.ptr, ctypes.c_int64(self.nverts), of.ptr, ctypes.c_int64(self.ntris),
                                                  ctypes.byref(nv), ctypes.byref(nt), None, self.stream), "mesh_keep_largest")
        return DeviceMesh(ov, nv.value, of, nt.value, self.stream, owns=True)

    def select_seeded(self, ids) -> "DeviceMesh":
        """the regions that hold any of the point ids `ids` (a host sequence, or a `DeviceBuffer` of int32 with `count`)"""
        from .device import DeviceBuffer
        seeds = _seed_ids(ids, self.nverts)  # (raises before anything is launched)
        sbuf = DeviceBuffer(seeds.nbytes + 16)
        ov, of = DeviceBuffer(self.nverts * 12 + 16), DeviceBuffer(self.ntris * 12 + 16)
        nv, nt = ctypes.c_int64(0), ctypes.c_int64(0)
        try:
            if len(seeds):
                sbuf.upload(seeds)
            L.check(L.lib().ivx_dev_mesh_select_seeded(self.verts.ptr, ctypes.c_int64(self.nverts), self.faces.ptr,
                                                       ctypes.c_int64(self.ntris), sbuf.ptr, ctypes.c_int64(len(seeds)), ov.ptr,
                                                       ctypes.c_int64(self.nverts), of.ptr, ctypes.c_int64(self.ntris), ctypes.byref(nv),
                                                       ctypes.byref(nt), self.stream), "mesh_select_seeded")
        finally:
            sbuf.close()  # (the call waited for its counts: the seeds have been read)
        return DeviceMesh(ov, nv.value, of, nt.value, self.stream, owns=True)

    def nearest_point(self, xyz) -> int:
        """id of the point nearest to `xyz` (float64 distances, the smallest id on a tie); -1 for a mesh without points"""
        from .device import DeviceBuffer
        q = (ctypes.c_double * 3)(*[float(x) for x in xyz])
        out = DeviceBuffer(16)
        try:
            L.check(L.lib().ivx_dev_mesh_nearest_point(self.verts.ptr, ctypes.c_int64(self.nverts), q, out.ptr, self.stream),
                    "mesh_nearest_point")
            self.sync()
            return int(out.download((1,), np.int32)[0])
        finally:
            out.close()

    def split(self) -> "MeshParts":
        from .device import DeviceBuffer
        lib = L.lib()
        nv, nr = ctypes.c_int64(0), ctypes.c_int64(0)
        args = (self.verts.ptr, ctypes.c_int64(self.nverts), self.faces.ptr, ctypes.c_int64(self.ntris))
        L.check(lib.ivx_dev_mesh_split(*args, None, ctypes.c_int64(0), None, ctypes.c_int64(0), None, ctypes.c_int64(0),
                                       ctypes.byref(nv), ctypes.byref(nr), self.stream), "mesh_split")
        ov, of, tb = DeviceBuffer(nv.value * 12 + 16), DeviceBuffer(self.ntris * 12 + 16), DeviceBuffer(nr.value * 32 + 16)
        if nr.value:
            L.check(lib.ivx_dev_mesh_split(*args, ov.ptr, nv, of.ptr, ctypes.c_int64(self.ntris), tb.ptr, nr, ctypes.byref(nv),
                                           ctypes.byref(nr), self.stream), "mesh_split")
        return MeshParts(ov, nv.value, of, self.ntris if nr.value else 0, tb, nr.value, self.stream)

    # ---- the geodesic measure ----
    def graph(self):
        """the mesh graph (unique neighbours per point, ascending, CSR) as a `DeviceBuffer`: built on first use, kept until
        `close`, read by every measure on this mesh"""
        if self._graph is None:
            from .device import DeviceBuffer
            nbytes = ctypes.c_size_t(0)
            L.check(L.lib().ivx_mesh_graph_bytes(ctypes.c_int64(self.nverts), ctypes.c_int64(self.ntris), ctypes.byref(nbytes)),
                    "mesh_graph_bytes")
            g = DeviceBuffer(nbytes.value)
            try:
                L.check(L.lib().ivx_dev_mesh_graph_build(self.faces.ptr, ctypes.c_int64(self.nverts), ctypes.c_int64(self.ntris), g.ptr,
                                                         ctypes.c_size_t(nbytes.value), self.stream), "mesh_graph_build")
            except Exception:
                g.close()
                raise
            self._graph = g
        return self._graph

    def graph_arrays(self):
        """``(offsets uint32 (V + 1,), neighbours uint32 (E,))`` of `graph`, downloaded"""
        g = self.graph()
        self.sync()
        head = g.download((32,), np.int64)
        if int(head[1]) != self.nverts or int(head[2]) != self.ntris:
            raise RuntimeError("mesh graph: header does not describe this mesh")
        ne, at_off, at_adj = int(head[3]), int(head[4]), int(head[5])
        off, adj = np.empty(self.nverts + 1, np.uint32), np.empty(ne, np.uint32)
        L.check(L.lib().ivx_memcpy_d2h(L.ptr(off), g.at(at_off), ctypes.c_size_t(off.nbytes)))
        if ne:
            L.check(L.lib().ivx_memcpy_d2h(L.ptr(adj), g.at(at_adj), ctypes.c_size_t(adj.nbytes)))
        return off, adj

    def geodesic_distances(self, source, stop_at=None, delta=None, rounds_per_look=None, with_stats=False):
        """``(dist float64 (V,), pred int32 (V,))`` from point `source` along the triangle edges (ivx.h: +inf / -1 where the
        source does not reach; with `stop_at` the entries above ``dist[stop_at]`` are upper bounds).  `delta` /
        `rounds_per_look`: the schedule, None for the library's default -- neither changes a bit of `dist`.
        `with_stats` adds the dict of rounds, relaxations, threshold advances and host looks."""
        from .device import DeviceBuffer
        source, stop = _point_id(source, self.nverts, "source"), -1 if stop_at is None else _point_id(stop_at, self.nverts, "stop_at")
        graph = self.graph()
        d, p = DeviceBuffer(self.nverts * 8 + 16), DeviceBuffer(self.nverts * 4 + 16)
        stats = (ctypes.c_int64 * 4)()
        try:
            L.check(L.lib().ivx_dev_mesh_geodesic_distances(self.verts.ptr, ctypes.c_int64(self.nverts), graph.ptr, ctypes.c_int64(source),
                                                            ctypes.c_int64(stop), ctypes.c_double(0.0 if delta is None else float(delta)),
                                                            ctypes.c_int(0 if rounds_per_look is None else int(rounds_per_look)),
                                                            d.ptr, p.ptr, stats, self.stream), "mesh_geodesic_distances")
            self.sync()
            out = d.download((self.nverts,), np.float64), p.download((self.nverts,), np.int32)
        finally:
            d.close()
            p.close()
        return out + (_geo_stats(stats),) if with_stats else out

    def geodesic(self, points=None, ids=None) -> "GeodesicPath":
        """The shortest path along the triangle edges through two or more picks, in order: `points` are coordinates, each
        snapped with `nearest_point` (the reference's vtkPointLocator.FindClosestPoint), or `ids` the point ids themselves."""
        from .device import DeviceBuffer
        if (points is None) == (ids is None):
            raise ValueError("geodesic: give points or ids")
        if ids is None:
            pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
            if len(pts) < 2:
                raise ValueError("geodesic: at least two points needed")
            if self.nverts == 0:
                raise ValueError("geodesic: the mesh has no points")
            ids = [self.nearest_point(xyz) for xyz in pts]
        ids = geodesic_ids(ids, self.nverts)
        nseg = len(ids) - 1
        graph = self.graph()
        room = max(self.nverts, 1) * nseg
        path = DeviceBuffer(room * 4 + 16)
        seg_n, seg_len, stats = (ctypes.c_int64 * nseg)(), (ctypes.c_double * nseg)(), (ctypes.c_int64 * 4)()
        try:
            L.check(L.lib().ivx_dev_mesh_geodesic_path(self.verts.ptr, ctypes.c_int64(self.nverts), graph.ptr, L.ptr(ids),
                                                       ctypes.c_int64(len(ids)), path.ptr, ctypes.c_int64(room), seg_n, seg_len, stats,
                                                       self.stream), "mesh_geodesic_path")
            self.sync()
            total = int(sum(seg_n))
            flat = path.download((total,), np.int32) if total else np.zeros(0, np.int32)
            coords = np.zeros((total, 3), np.float32)
            if total:
                whole = self.verts.download((self.nverts, 3), np.float32)
                coords = whole[flat]
        finally:
            path.close()
        cuts = np.cumsum([0] + [int(n) for n in seg_n])
        return GeodesicPath([flat[cuts[q]:cuts[q + 1]].copy() for q in range(nseg)], np.ascontiguousarray(coords),
                            [float(x) for x in seg_len], ids, _geo_stats(stats))

    # ---- surface view ----
    def render(self, normals=None, colour=None, transparency=0.0, **kwargs):
        """A shaded picture of this mesh alone: `surface_view.Scene.render` (whose keywords these are, ``download=False``
        apart) of one actor; `normals`: a device buffer of one float32 normal per point, or None (flat shading)."""
        from . import surface_view as sv
        actor = sv.SurfaceActor(self, normals=normals, colour=sv.SURFACE_COLOUR[0] if colour is None else colour, transparency=transparency)
        with sv.Scene([actor], self.stream) as scene:
            return scene.render(download=True, **kwargs)

    def close(self):
        if self._graph is not None:
            self._graph.close()
            self._graph = None
        if self._owns:
            self.verts.close()
            self.faces.close()
        self._owns = False


class GeodesicPath:
    """What `DeviceMesh.geodesic` returns.  `ids`: one int32 array per segment, from its start to its end (empty when the end
    cannot be reached, one id when start == end); `points`: float32 (n, 3), the segments' coordinates one after the other, the
    joints repeated the way vtkAppendPolyData repeats them; `segment_lengths`: ``dist[end]`` per segment (+inf when
    unreachable); `length`: the sum of the finite ones, in order; `point_ids`: the picks' ids; `stats`."""

    def __init__(self, ids, points, segment_lengths, point_ids, stats):
        self.ids, self.points, self.segment_lengths, self.point_ids, self.stats = ids, points, segment_lengths, point_ids, stats
        total = 0.0
        for x in segment_lengths:
            if math.isfinite(x):
                total += x
        self.length = total


def _geo_stats(stats) -> dict:
    return {"rounds": int(stats[0]), "relaxations": int(stats[1]), "threshold_advances": int(stats[2]), "host_looks": int(stats[3])}


def _point_id(i, nverts, what) -> int:
    if isinstance(i, bool) or not isinstance(i, (int, np.integer)):
        raise ValueError("%s must be an integer point id" % what)
    if not 0 <= int(i) < int(nverts):
        raise ValueError("%s %d outside [0, %d)" % (what, int(i), int(nverts)))
    return int(i)


def geodesic_ids(ids, nverts) -> np.ndarray:
    """the picks' ids as int32, checked on the host before anything runs: fewer than two, or an id outside [0, nverts), is a
    ValueError"""
    a = np.asarray(list(ids) if not isinstance(ids, np.ndarray) else ids)
    if a.size < 2:
        raise ValueError("geodesic: at least two points needed")
    if a.dtype.kind not in "iu":
        raise ValueError("geodesic: point ids must be integers")
    a = a.reshape(-1).astype(np.int64)
    if a.min() < 0 or a.max() >= int(nverts):
        bad = a[(a < 0) | (a >= int(nverts))][0]
        raise ValueError("geodesic: point id %d outside [0, %d)" % (int(bad), int(nverts)))
    return np.ascontiguousarray(a, dtype=np.int32)


def _seed_ids(ids, nverts) -> np.ndarray:
    """the seed list as int32, checked on the host: an id outside [0, nverts) is a ValueError (VTK skips negative ids
    and reads past its array for large ones)"""
    a = np.asarray(list(ids) if not isinstance(ids, np.ndarray) else ids)
    if a.size == 0:
        return np.zeros(0, np.int32)
    if a.dtype.kind not in "iu":
        raise ValueError("seed point ids must be integers")
    a = a.reshape(-1).astype(np.int64)
    if a.min() < 0 or a.max() >= int(nverts):
        bad = a[(a < 0) | (a >= int(nverts))][0]
        raise ValueError("seed point id %d outside [0, %d)" % (int(bad), int(nverts)))
    return np.ascontiguousarray(a, dtype=np.int32)


class _BufferView:
    """A window into a `DeviceBuffer` that somebody else owns: same calls, `close` does nothing.  Only 4-byte aligned."""

    def __init__(self, base, offset_bytes: int, nbytes: int):
        self._base, self.nbytes = base, int(nbytes)
        self.ptr = ctypes.c_void_p(base.ptr.value + int(offset_bytes))

    def download(self, shape, dtype, out=None):
        if out is None:
            out = np.empty(shape, dtype)
        assert out.flags["C_CONTIGUOUS"] and out.nbytes <= self.nbytes
        if out.nbytes:
            L.check(L.lib().ivx_memcpy_d2h(L.ptr(out), self.ptr, ctypes.c_size_t(out.nbytes)))
        return out

    def at(self, offset_bytes: int):
        return ctypes.c_void_p(self.ptr.value + int(offset_bytes))

    def close(self):
        pass


class MeshParts:
    """Every connected part of a mesh, resident (``DeviceMesh.split``): all triangles grouped by region with part-local point
    ids, the used points grouped the same way, and the part table -- `table` on the host, ``int64 (R, 4)`` = (triangle offset,
    triangles, point offset, points)."""

    def __init__(self, verts_buf, nverts, faces_buf, ntris, table_buf, n, stream=None):
        self.verts, self.nverts, self.faces, self.ntris, self.table_buf, self.n, self.stream = (
            verts_buf, int(nverts), faces_buf, int(ntris), table_buf, int(n), stream)
        self._table = None

    def sync(self):
        L.check(L.lib().ivx_stream_synchronize(self.stream) if self.stream else L.lib().ivx_device_synchronize())

    @property
    def table(self) -> np.ndarray:
        if self._table is None:
            self.sync()
            self._table = self.table_buf.download((self.n, 4), np.int64) if self.n else np.zeros((0, 4), np.int64)
        return self._table

    def part(self, i: int) -> DeviceMesh:
        """part `i` as a `DeviceMesh` that looks into the grouped buffers (valid until `close`; 4-byte aligned: every mesh
        kernel loads single floats / ints)"""
        to, tn, vo, vn = (int(x) for x in self.table[int(i)])
        return DeviceMesh(_BufferView(self.verts, vo * 12, vn * 12), vn, _BufferView(self.faces, to * 12, tn * 12), tn, self.stream)

    def download(self, i: int):
        return self.part(i).download()

    def mass_properties(self, small_max: int = 0) -> np.ndarray:
        """``float64 (R, 2)``: volume and area of every part (`surface_process.mass_properties` of each)"""
        return self.mass_properties_full(small_max)[:, :2].copy()

    def mass_properties_full(self, small_max: int = 0) -> np.ndarray:
        from .device import DeviceBuffer
        if not self.n:
            return np.zeros((0, 8), np.float64)
        out = DeviceBuffer(self.n * 64 + 16)
        try:
            L.check(L.lib().ivx_dev_mesh_parts_mass(self.verts.ptr, self.faces.ptr, self.table_buf.ptr, ctypes.c_int64(self.n),
                                                    ctypes.c_int64(self.ntris), ctypes.c_int64(int(small_max)), out.ptr, self.stream),
                    "mesh_parts_mass")
            self.sync()
            return out.download((self.n, 8), np.float64)
        finally:
            out.close()

    def close(self):
        for b in (self.verts, self.faces, self.table_buf):
            if b is not None:
                b.close()
        self.verts = self.faces = self.table_buf = None


def bounds(verts) -> tuple:
    """``(xmin, xmax, ymin, ymax, zmin, zmax)`` over ALL points, used by a triangle or not (vtkPolyData.GetBounds); zeros for
    an empty mesh."""
    if isinstance(verts, DeviceMesh):
        return verts.bounds()
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(6, np.float32)
    L.check(L.lib().ivx_mesh_bounds(L.ptr(v), ctypes.c_int64(len(v)), L.ptr(out)), "mesh_bounds")
    return tuple(float(x) for x in out)


def depth_buffer(verts, faces, view, size=None) -> np.ndarray:
    """The float32 z-buffer ``(H, W)`` of one view (a dict as `views_for_positions` makes them; `size`, when given, must be the
    view's): 1.0 where nothing is drawn, row 0 at the bottom of the viewport."""
    v, f = _mesh(verts, faces)
    w_px, h_px = view["size"]
    if size is not None and (int(size[0]), int(size[1])) != (w_px, h_px):
        raise ValueError("size %r is not the view's %r" % (tuple(size), (w_px, h_px)))
    out = np.empty((h_px, w_px), np.float32)
    L.check(L.lib().ivx_mesh_depth_raster(L.ptr(v), ctypes.c_int64(len(v)), L.ptr(f), ctypes.c_int64(len(f)), _c_views([view]),
                                          L.ptr(out)), "mesh_depth_raster")
    return out


def visible_points(verts, faces=None, positions=POSITIONS, size=SIZE, views=None) -> np.ndarray:
    """uint8 flag per point: 1 when any of the views sees it (inside the viewport and no deeper than the z-buffer + 0.01, the
    default tolerance of vtkSelectVisiblePoints).  `views` overrides the cameras made from the bounds and `positions`."""
    if isinstance(verts, DeviceMesh):
        m = verts
        if views is None:
            views = views_for_positions(m.bounds(), positions, size)
        flags = m.visible_flags(views)
        try:
            m.sync()
            return flags.download((m.nverts,), np.uint8)
        finally:
            flags.close()
    v, f = _mesh(verts, faces)
    if views is None:
        views = views_for_positions(bounds(v), positions, size)
    out = np.zeros(len(v), np.uint8)
    L.check(L.lib().ivx_mesh_visible_points(L.ptr(v), ctypes.c_int64(len(v)), L.ptr(f), ctypes.c_int64(len(f)), _c_views(views),
                                            len(views), L.ptr(out)), "mesh_visible_points")
    return out


def select_by_point_flags(verts, faces, flags, invert=False):
    """The triangles with ANY corner flagged (`invert`: any corner not flagged), in order, on the points they use, compacted in
    order (the ``GetPointCells`` union + vtkExtractSelection of polydata_utils.py:420-449)."""
    v, f = _mesh(verts, faces)
    fl = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    if len(fl) != len(v):
        raise ValueError("one flag per point")
    ov, of = np.empty_like(v), np.empty_like(f)
    nv, nt = ctypes.c_int64(0), ctypes.c_int64(0)
    L.check(L.lib().ivx_mesh_select_points(L.ptr(v), ctypes.c_int64(len(v)), L.ptr(f), ctypes.c_int64(len(f)), L.ptr(fl),
                                           int(bool(invert)), L.ptr(ov), L.ptr(of), ctypes.byref(nv), ctypes.byref(nt)),
            "mesh_select_points")
    return ov[: nv.value].copy(), of[: nt.value].copy()


def RemoveNonVisibleFaces(verts, faces=None, positions=POSITIONS, remove_visible=False, size=SIZE):
    """``pu.RemoveNonVisibleFaces`` (:363-455): keeps the triangles that touch a visible point -- or, with `remove_visible`,
    those that touch a hidden one (the reference's naming: a triangle with corners of both kinds is in both results).
    Arrays in -> ``(verts', faces')``; a `DeviceMesh` in (``faces=None``) -> a `DeviceMesh` out, nothing downloaded."""
    if isinstance(verts, DeviceMesh):
        m = verts
        views = views_for_positions(m.bounds(), positions, size)
        flags = m.visible_flags(views)
        try:
            return m.select(flags, remove_visible)
        finally:
            flags.close()
    v, f = _mesh(verts, faces)
    views = views_for_positions(bounds(v), positions, size)
    ov, of = np.empty_like(v), np.empty_like(f)
    nv, nt = ctypes.c_int64(0), ctypes.c_int64(0)
    L.check(L.lib().ivx_mesh_remove_nonvisible(L.ptr(v), ctypes.c_int64(len(v)), L.ptr(f), ctypes.c_int64(len(f)), _c_views(views),
                                               len(views), int(bool(remove_visible)), L.ptr(ov), L.ptr(of), ctypes.byref(nv),
                                               ctypes.byref(nt)), "mesh_remove_nonvisible")
    return ov[: nv.value].copy(), of[: nt.value].copy()


def HasNonVisibleFaces(verts, faces=None, threshold=0.7, positions=POSITIONS, size=SIZE) -> bool:
    """``pu.HasNonVisibleFaces`` (:281-360): True when fewer than `threshold` of the points are visible; False for an empty
    mesh."""
    n = verts.nverts if isinstance(verts, DeviceMesh) else len(np.asarray(verts).reshape(-1, 3))
    if n == 0:
        return False
    return int(np.count_nonzero(visible_points(verts, faces, positions, size))) / n < threshold


# ---- surface connectivity (polydata_utils.py:206-278) ----
def split_arrays(verts, faces):
    """The split on host arrays in one piece: ``(grouped verts, grouped faces with part-local ids, table int64 (R, 4))``."""
    v, f = _mesh(verts, faces)
    lib = L.lib()
    nv, nr = ctypes.c_int64(0), ctypes.c_int64(0)
    args = (L.ptr(v), ctypes.c_int64(len(v)), L.ptr(f), ctypes.c_int64(len(f)))
    L.check(lib.ivx_mesh_split(*args, None, None, None, ctypes.byref(nv), ctypes.byref(nr)), "mesh_split")
    ov, of, tb = np.empty((nv.value, 3), np.float32), np.empty((len(f), 3), np.int32), np.empty((nr.value, 4), np.int64)
    if nr.value:
        L.check(lib.ivx_mesh_split(*args, L.ptr(ov), L.ptr(of), L.ptr(tb), ctypes.byref(nv), ctypes.byref(nr)), "mesh_split")
    return ov, of, tb


def parts_mass_properties(verts, faces, table) -> np.ndarray:
    """``float64 (R, 2)`` volume and area of every part of a grouped mesh (what `split_arrays` returns)"""
    v, f = _mesh(verts, faces)
    tb = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 4)
    out = np.zeros((len(tb), 8), np.float64)
    L.check(L.lib().ivx_mesh_parts_mass(L.ptr(v), ctypes.c_int64(len(v)), L.ptr(f), ctypes.c_int64(len(f)), L.ptr(tb),
                                        ctypes.c_int64(len(tb)), L.ptr(out)), "mesh_parts_mass")
    return out[:, :2].copy()


def nearest_point(verts, xyz) -> int:
    """id of the point nearest to `xyz` (float64 distances, the smallest id on a tie); -1 without points"""
    if isinstance(verts, DeviceMesh):
        return verts.nearest_point(xyz)
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    q = (ctypes.c_double * 3)(*[float(x) for x in xyz])
    out = ctypes.c_int64(-1)
    L.check(L.lib().ivx_mesh_nearest_point(L.ptr(v), ctypes.c_int64(len(v)), q, ctypes.byref(out)), "mesh_nearest_point")
    return int(out.value)


def SplitDisconectedParts(verts, faces=None):
    """``pu.SplitDisconectedParts`` (:241-278): every connected part, in region order (region r = the r-th region in the order of
    its first triangle, the `r` of AddSpecifiedRegion).  A part keeps its triangles in their original order, on the points they
    use in original order.  Arrays in -> a list of ``(verts, faces)``; a `DeviceMesh` in -> `MeshParts`, nothing downloaded."""
    if isinstance(verts, DeviceMesh):
        return verts.split()
    ov, of, tb = split_arrays(verts, faces)
    return [(ov[vo:vo + vn].copy(), of[to:to + tn].copy()) for to, tn, vo, vn in tb.tolist()]


def JoinSeedsParts(verts, faces=None, point_id_list=()):
    """``pu.JoinSeedsParts`` (:206-238): the union of the regions that hold any of the seed point ids.  Duplicate seeds are
    harmless, a seed no triangle uses selects nothing, no seeds give an empty mesh; a seed outside ``[0, len(verts))`` is a
    ValueError, raised before anything runs on the GPU (DEVIATION: VTK skips negative ids and reads past its array for large
    ones).  Arrays in -> ``(verts', faces')``; a `DeviceMesh` in (``faces=None``) -> a `DeviceMesh` out."""
    if isinstance(verts, DeviceMesh):
        return verts.select_seeded(point_id_list)
    v, f = _mesh(verts, faces)
    seeds = _seed_ids(point_id_list, len(v)).astype(np.int64)
    ov, of = np.empty_like(v), np.empty_like(f)
    nv, nt = ctypes.c_int64(0), ctypes.c_int64(0)
    L.check(L.lib().ivx_mesh_select_seeded(L.ptr(v), ctypes.c_int64(len(v)), L.ptr(f), ctypes.c_int64(len(f)), L.ptr(seeds),
                                           ctypes.c_int64(len(seeds)), L.ptr(ov), L.ptr(of), ctypes.byref(nv), ctypes.byref(nt)),
            "mesh_select_seeded")
    return ov[: nv.value].copy(), of[: nt.value].copy()


def SelectLargestPart(verts, faces=None):
    """``pu.SelectLargestPart`` (:188-203): the part with the most triangles, the earliest on a tie
    (`surface_process.keep_largest`)."""
    if isinstance(verts, DeviceMesh):
        return verts.keep_largest()
    from . import surface_process as sp
    return sp.keep_largest(verts, faces)[:2]
