"""``invesalius.data.measures`` -- the geodesic measure on the GPU (csrc/k_meshgeo.hip).

``GeodesicMeasure._draw_line`` (measures.py:1202-1256) snaps every pick to its nearest mesh point
(vtkPointLocator.FindClosestPoint), lets vtkDijkstraGraphGeodesicPath walk the triangle edges between consecutive picks and
shows the summed edge length in mm.  Here the surface is arrays or a resident `polydata_utils.DeviceMesh`, the snap is
``nearest_point`` and the paths come from ``DeviceMesh.geodesic``; the class below is the host mirror of the reference's,
without its actors (points, tube, text).

PARITY UNPINNED vs VTK; distances pinned to scipy.sparse.csgraph.dijkstra bit for bit (tests/test_gpu_geodesic.py).  The
reference adds every edge of every segment into one running double; `length` here is the in-order sum of the segments'
``dist[end]``, each of which equals the sum of its own edges from its start.  The two can differ in the last bits."""
from __future__ import annotations

import math

import numpy as np

from . import _lib as L
from . import polydata_utils as pu


def _picks(points) -> np.ndarray:
    p = np.asarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("geodesic: points must be rows of x y z")
    if len(p) < 2:
        raise ValueError("geodesic: at least two points needed")
    if not np.isfinite(p).all():
        raise ValueError("geodesic: points must be finite")
    return p


def geodesic_path(verts, faces=None, points=None, ids=None) -> "pu.GeodesicPath":
    """The geodesic through the picks `points` (coordinates, snapped to their nearest mesh points) or `ids` (the point ids
    themselves) on the surface ``verts`` float32 (N, 3) / ``faces`` int32 (T, 3), or on a `DeviceMesh` (``faces=None``).
    Fewer than two picks, an id outside ``[0, N)`` or a face index outside it is a ValueError, raised before the library is
    touched; without a HIP device the call is a RuntimeError."""
    if (points is None) == (ids is None):
        raise ValueError("geodesic: give points or ids")
    if isinstance(verts, pu.DeviceMesh):
        mesh, own = verts, False
        nverts = mesh.nverts
    else:
        v, f = pu._mesh(verts, faces if faces is not None else np.zeros((0, 3), np.int32))
        if len(f) and (f.min() < 0 or f.max() >= len(v)):
            raise ValueError("mesh: face index outside [0, %d)" % len(v))
        mesh, own, nverts = None, True, len(v)
    if ids is not None:
        ids = pu.geodesic_ids(ids, nverts)
    else:
        points = _picks(points)
        if nverts == 0:
            raise ValueError("geodesic: the mesh has no points")
    L.require_device()
    if own:
        mesh = pu.DeviceMesh.upload(v, f)
    try:
        return mesh.geodesic(points=points, ids=ids)
    finally:
        if own:
            mesh.close()


class GeodesicMeasure:
    """The reference's ``GeodesicMeasure`` (measures.py:1068-1282) without actors.  ``SetSurface`` takes arrays (uploaded, owned
    and freed by `close`) or a `DeviceMesh` (borrowed); the surface's graph is built once and serves every recomputation.  The
    path is recomputed whenever a point changes while two or more are set.  An unreachable segment is skipped, as the reference's
    ``if path_segment.GetNumberOfPoints() > 0`` skips it."""

    def __init__(self, multi_point: bool = False):
        self.points = []
        self.multi_point = bool(multi_point)  # the session's "geodesic_multi_point"
        self.mesh = None
        self._owns_mesh = False
        self._is_finalized = False
        self._path_computed = False
        self._path_length = 0.0
        self.path = None  # the last `polydata_utils.GeodesicPath`

    def SetSurface(self, verts, faces=None):
        self._drop_mesh()
        if verts is None:
            pass
        elif isinstance(verts, pu.DeviceMesh):
            self.mesh = verts
        else:
            L.require_device()
            self.mesh, self._owns_mesh = pu.DeviceMesh.upload(verts, faces), True
        self._recompute()

    def SetPoint1(self, x, y, z):
        if not self.points:
            self.points.append((float(x), float(y), float(z)))
        else:
            self.points[0] = (float(x), float(y), float(z))
        self._recompute()

    def SetPoint2(self, x, y, z):
        if not self.points:
            raise ValueError("geodesic measure: the first point is not set")
        if len(self.points) == 1:
            self.points.append((float(x), float(y), float(z)))
        else:
            self.points[1] = (float(x), float(y), float(z))
        self._recompute()

    def AddPoint(self, x, y, z) -> bool:
        """the next pick; in two-point mode a third one is ignored (False), as the reference returns no actor for it"""
        if not self.multi_point and len(self.points) >= 2:
            return False
        self.points.append((float(x), float(y), float(z)))
        self._recompute()
        return True

    def finalize(self):
        self._is_finalized = True

    def IsComplete(self, multi_point=None) -> bool:
        if self.multi_point if multi_point is None else multi_point:
            return self._is_finalized
        return len(self.points) >= 2

    def GetValue(self) -> float:
        """the geodesic length in mm once a path exists, the straight-line distance of the first two points before that"""
        if self._path_computed:
            return self._path_length
        if len(self.points) >= 2:
            p, q = self.points[0], self.points[1]
            return math.sqrt((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 + (p[2] - q[2]) ** 2)
        return 0.0

    def GetNumberOfPoints(self) -> int:
        return len(self.points)

    def _recompute(self):
        self._path_computed, self._path_length, self.path = False, 0.0, None
        if self.mesh is None or self.mesh.ntris == 0 or len(self.points) < 2:
            return
        self.path = self.mesh.geodesic(points=_picks(self.points))
        if len(self.path.points) == 0:  # (the reference returns before it stores a length: no segment was reachable)
            return
        self._path_length = self.path.length
        self._path_computed = True

    def _drop_mesh(self):
        if self.mesh is not None and self._owns_mesh:
            self.mesh.close()
        self.mesh, self._owns_mesh = None, False

    def close(self):
        self._drop_mesh()
