"""``invesalius.data.measures`` -- the geodesic measure (csrc/k_meshgeo.hip) and the density measures
(csrc/k_density_roi.hip; below the geodesic measure in this file) on the GPU.

``GeodesicMeasure._draw_line`` (measures.py:1202-1256) snaps every pick to its nearest mesh point
(vtkPointLocator.FindClosestPoint), lets vtkDijkstraGraphGeodesicPath walk the triangle edges between consecutive picks and
shows the summed edge length in mm.  Here the surface is arrays or a resident `polydata_utils.DeviceMesh`, the snap is
``nearest_point`` and the paths come from ``DeviceMesh.geodesic``; the class below is the host mirror of the reference's,
without its actors (points, tube, text).

PARITY UNPINNED vs VTK; distances pinned to scipy.sparse.csgraph.dijkstra bit for bit (tests/test_gpu_geodesic.py).  The
reference adds every edge of every segment into one running double; `length` here is the in-order sum of the segments'
``dist[end]``, each of which equals the sum of its own edges from its start.  The two can differ in the last bits."""
from __future__ import annotations

import ctypes
import itertools
import math
from fractions import Fraction

import numpy as np

from . import _lib as L
from . import math_utils
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


# ---- the density measures ---------------------------------------------------------------------------------------
# ``CircleDensityMeasure`` / ``PolygonDensityMeasure`` (measures.py:1818-2420) without canvas, handles or actors, the records
# ``Measurement`` / ``DensityMeasurement`` (measures.py:673-771) and the batched call the panel needs.  Which pixels a measure
# selects: rule E (the reference's ellipse, bit for bit) and rule P (PARITY UNPINNED vs wx: the reference fills the polygon
# through a wx GraphicsContext, which is not available to this project; the pinned rule is the odd-even crossing test of
# polygon2mask_rs at the pixel's centre).  Both are stated in csrc/density_roi_math.h.  Rule E puts pixel i at i * spacing,
# rule P at i + 0.5: the half pixel between them is the reference's.

# invesalius/constants.py: locations, measure types, the name pattern and the colour cycle
AXIAL, CORONAL, SAGITAL, VOLUME, SURFACE = 1, 2, 3, 4, 5
LINEAR, ANGULAR, DENSITY_ELLIPSE, DENSITY_POLYGON = 6, 7, 8, 9
ORIENTATIONS = {AXIAL: "AXIAL", CORONAL: "CORONAL", SAGITAL: "SAGITAL"}
LOCATIONS = {v: k for k, v in ORIENTATIONS.items()}
MEASURE_NAME_PATTERN = "M %d"
MEASURE_COLOUR = itertools.cycle([[1, 0, 0], [1, 0.4, 0], [0, 0, 1], [1, 0, 1], [0, 0.6, 0]])
_AXIS = {"AXIAL": 0, "CORONAL": 1, "SAGITAL": 2}
# the two in-plane coordinates (of x, y, z) per orientation: columns, rows
_PLANE = {"AXIAL": (0, 1), "CORONAL": (0, 2), "SAGITAL": (1, 2)}


class Measurement:
    """the reference's record of a linear / angular measure (measures.py:673-711), same keys"""
    general_index = -1

    def __init__(self):
        Measurement.general_index += 1
        self.index = Measurement.general_index
        self.name = MEASURE_NAME_PATTERN % (self.index + 1)
        self.colour = next(MEASURE_COLOUR)
        self.value = 0
        self.location = SURFACE
        self.type = LINEAR
        self.slice_number = 0
        self.points = []
        self.visible = True

    _KEYS = ("index", "name", "colour", "value", "location", "type", "slice_number", "points", "visible")

    def Load(self, info):
        for key in self._KEYS:
            setattr(self, key, info[key])

    def get_as_dict(self):
        return {key: getattr(self, key) for key in self._KEYS}


class DensityMeasurement:
    """the reference's record of a density measure (measures.py:714-771).  Its quirks are kept: a fresh record has no
    ``value`` until a density was computed (or `Load` ran), `get_as_dict` writes no "perimeter", `Load` tolerates its absence."""
    general_index = -1

    def __init__(self):
        DensityMeasurement.general_index += 1
        self.index = DensityMeasurement.general_index
        self.name = MEASURE_NAME_PATTERN % (self.index + 1)
        self.colour = next(MEASURE_COLOUR)
        self.area = 0
        self.perimeter = 0.0
        self.min = 0
        self.max = 0
        self.mean = 0
        self.std = 0
        self.location = AXIAL
        self.type = DENSITY_ELLIPSE
        self.slice_number = 0
        self.points = []
        self.visible = True

    _KEYS = ("index", "name", "colour", "value", "location", "type", "slice_number", "points", "visible", "area", "min", "max", "mean", "std")

    def Load(self, info):
        for key in self._KEYS:
            setattr(self, key, info[key])
        self.perimeter = info.get("perimeter", 0.0)

    def get_as_dict(self):
        return {key: getattr(self, key) for key in self._KEYS}


class _Grid:
    """where the int16 voxels are: the address of voxel [0][0][0], the shape and the byte strides (host array or device block)"""

    def __init__(self, base: int, shape, strides):
        self.base, self.shape, self.strides = int(base), tuple(int(v) for v in shape), tuple(int(v) for v in strides)

    @classmethod
    def of(cls, image: np.ndarray):
        if not isinstance(image, np.ndarray) or image.dtype != np.int16 or image.ndim not in (2, 3):
            raise TypeError("image must be a 2-D or 3-D int16 array")
        if image.ndim == 2:  # a plain slice: the one axial slice of a volume of depth 1
            return cls(image.ctypes.data, (1,) + image.shape, (0,) + image.strides)
        return cls(image.ctypes.data, image.shape, image.strides)

    def view(self, orientation: str, n: int):
        """(address, row stride, element stride, h, w) of slice `n`, what Slice.get_image_slice returns for it"""
        ax = _AXIS.get(orientation)
        if ax is None:
            raise ValueError("orientation must be AXIAL, CORONAL or SAGITAL")
        if not 0 <= int(n) < self.shape[ax]:
            raise IndexError("slice %d outside the volume" % n)
        r, e = (a for a in range(3) if a != ax)
        return self.base + int(n) * self.strides[ax], self.strides[r], self.strides[e], self.shape[r], self.shape[e]


def _ogrid_length(n: int, step: float) -> int:
    """the length ``np.ogrid[0 : n * step : step]`` gives its axis: ceil(stop / step), which is n + 1 for some steps"""
    return int(math.ceil((n * step - 0) / (step * 1.0)))


class CircleDensityMeasure:
    """The reference's ellipse density measure (measures.py:1818-2119) without canvas: `center`, `point1` (its x -- or y, for
    SAGITAL -- gives the first radius) and `point2` (the second radius) are (x, y, z) in mm."""

    def __init__(self, orientation: str, slice_number: int, center=(0.0, 0.0, 0.0), point1=(0.0, 0.0, 0.0), point2=(0.0, 0.0, 0.0)):
        if orientation not in _AXIS:
            raise ValueError("orientation must be AXIAL, CORONAL or SAGITAL")
        self.orientation, self.slice_number = orientation, int(slice_number)
        self.center, self.point1, self.point2 = tuple(center), tuple(point1), tuple(point2)
        self._measurement = None
        self._min = self._max = self._mean = self._std = self._area = self._perimeter = 0

    def set_measurement(self, dm: DensityMeasurement):
        self._measurement = dm

    def _radii(self):
        i, j = _PLANE[self.orientation]
        return abs(self.point1[i] - self.center[i]), abs(self.point2[j] - self.center[j])

    def calc_area(self):
        return math_utils.calc_ellipse_area(*self._radii())

    def calc_perimeter(self) -> float:
        return math_utils.calc_ellipse_circumference(*self._radii())

    def _describe(self, grid: _Grid, spacing):
        """the library's descriptor of this measure on `grid` (rule E's parameters, picked as calc_density picks them)"""
        base, rs, es, h, w = grid.view(self.orientation, self.slice_number)
        i, j = _PLANE[self.orientation]
        sx, sy = spacing[i], spacing[j]
        if _ogrid_length(w, sx) != w or _ogrid_length(h, sy) != h:
            # np.ogrid makes such an axis one element longer than the slice, and the reference dies in img_slice[mask]
            raise IndexError("boolean index did not match indexed array: np.ogrid gives %d x %d for the %d x %d slice at spacing (%r, %r)"
                             % (_ogrid_length(h, sy), _ogrid_length(w, sx), h, w, sy, sx))
        a, b = self._radii()
        q = L.Roi(image=base, row_stride=rs, elem_stride=es, h=h, w=w, kind=L.ROI_ELLIPSE, sx=float(sx), sy=float(sy),
                  cx=float(self.center[i]), cy=float(self.center[j]), a2=float(a ** 2), b2=float(b ** 2))
        return q, None

    def _store(self, stats):
        _min, _max, _mean, _std = stats
        _area, _perimeter = self.calc_area(), self.calc_perimeter()
        if self._measurement:
            m = self._measurement
            m.points = [self.center, self.point1, self.point2]
            m.value = m.mean = float(_mean)
            m.min, m.max, m.std = float(_min), float(_max), float(_std)
            m.area, m.perimeter = float(_area), float(_perimeter)
        self._min, self._max, self._mean, self._std, self._area, self._perimeter = _min, _max, _mean, _std, _area, _perimeter
        return _result(_min, _max, _mean, _std, _area, _perimeter)

    def calc_density(self, image, spacing):
        """min, max, mean, std, area, perimeter and value = mean of the selected pixels of `image` (int16, (dz, dy, dx), or a
        `DeviceVolume`), stored on the attached measurement as measures.py:2093-2107 stores them"""
        return density_of(image, spacing, [self])[0]


class PolygonDensityMeasure:
    """The reference's polygon density measure (measures.py:2122-2420) without canvas: `points` are (x, y, z) in mm."""

    def __init__(self, orientation: str, slice_number: int, points=()):
        if orientation not in _AXIS:
            raise ValueError("orientation must be AXIAL, CORONAL or SAGITAL")
        self.orientation, self.slice_number = orientation, int(slice_number)
        self.points = [tuple(p) for p in points]
        self._measurement = None
        self._min = self._max = self._mean = self._std = self._area = self._perimeter = 0

    def set_measurement(self, dm: DensityMeasurement):
        self._measurement = dm

    def insert_point(self, point):
        self.points.append(tuple(point))

    def _plane_points(self):
        i, j = _PLANE[self.orientation]
        return [(p[i], p[j]) for p in self.points]

    def calc_area(self):
        return math_utils.calc_polygon_area(self._plane_points())

    def calc_perimeter(self) -> float:
        return math_utils.calc_polygon_perimeter(self._plane_points())

    def _describe(self, grid: _Grid, spacing):
        base, rs, es, h, w = grid.view(self.orientation, self.slice_number)
        i, j = _PLANE[self.orientation]
        sx, sy = spacing[i], spacing[j]
        pts = np.array([(x / sx, y / sy) for x, y in self._plane_points()], dtype=np.float64).reshape(-1, 2)
        if len(pts) > L.ROI_MAX_POINTS:
            raise TypeError("a polygon of %d points (at most %d)" % (len(pts), L.ROI_MAX_POINTS))
        return L.Roi(image=base, row_stride=rs, elem_stride=es, h=h, w=w, kind=L.ROI_POLYGON, n_points=len(pts)), pts

    def _store(self, stats):
        _min, _max, _mean, _std = stats
        _area, _perimeter = self.calc_area(), self.calc_perimeter()
        if self._measurement:
            m = self._measurement
            m.points = self.points
            m.value = m.mean = float(_mean)
            m.min, m.max, m.std = float(_min), float(_max), float(_std)
            m.area = float(_area)
            # (measures.py:2314 keeps the perimeter on the measure, not on the record: kept, the record's dict has no such key)
        self._min, self._max, self._mean, self._std, self._area, self._perimeter = _min, _max, _mean, _std, _area, float(_perimeter)
        return _result(_min, _max, _mean, _std, _area, _perimeter)

    def calc_density(self, image, spacing):
        """as `CircleDensityMeasure.calc_density`, under rule P"""
        return density_of(image, spacing, [self])[0]


def _result(_min, _max, _mean, _std, _area, _perimeter):
    return {"min": float(_min), "max": float(_max), "mean": float(_mean), "std": float(_std), "area": float(_area),
            "perimeter": float(_perimeter), "value": float(_mean)}


def stats_from_record(record):
    """(min, max, mean, std) from the library's cnt, s1, s2, lo, hi.  Four zeros for an empty selection, as the reference's
    ``except ValueError`` gives them.  The mean is one float64 division (== np.mean while |s1| < 2^53, which a slice cannot
    exceed); the variance is the exact rational (cnt s2 - s1^2) / cnt^2 rounded to float64 once and std its square root, the
    rule of `slice_.calc_image_density`."""
    cnt, s1, s2, lo, hi = (int(v) for v in record)
    if cnt == 0:
        return 0, 0, 0, 0
    return lo, hi, float(s1) / float(cnt), math.sqrt(float(Fraction(cnt * s2 - s1 * s1, cnt * cnt)))


def measure_from_dict(info):
    """the measure a ``measurements.plist`` entry of type DENSITY_ELLIPSE / DENSITY_POLYGON describes, its record attached"""
    dm = DensityMeasurement()
    dm.Load(info)
    orientation = ORIENTATIONS.get(dm.location)
    if orientation is None:
        raise ValueError("density measure %r: location %r is no slice orientation" % (dm.name, dm.location))
    if dm.type == DENSITY_ELLIPSE:
        if len(dm.points) != 3:
            raise ValueError("density measure %r: an ellipse holds center, point1 and point2" % dm.name)
        m = CircleDensityMeasure(orientation, dm.slice_number, *dm.points)
    elif dm.type == DENSITY_POLYGON:
        m = PolygonDensityMeasure(orientation, dm.slice_number, dm.points)
    else:
        raise ValueError("measurement %r is no density measure (type %r)" % (dm.name, dm.type))
    m.set_measurement(dm)
    return m


def describe_rois(grid: _Grid, spacing, measures):
    """(the descriptor array, the points block (n, 2) float64) of `measures` on `grid`"""
    q = (L.Roi * max(len(measures), 1))()
    blocks, at = [], 0
    for k, m in enumerate(measures):
        d, pts = m._describe(grid, spacing)
        if pts is not None:
            d.first_point = at
            at += len(pts)
            blocks.append(pts)
        q[k] = d
    points = np.ascontiguousarray(np.concatenate(blocks)) if blocks else np.zeros((0, 2), np.float64)
    return q, points


def roi_records(q, n_rois: int, points: np.ndarray) -> np.ndarray:
    """ivx_roi_density: the (n_rois, 5) int64 records cnt, s1, s2, lo, hi of host views, one library call"""
    out = np.zeros((n_rois, 5), np.int64)
    if n_rois:
        L.check(L.lib().ivx_roi_density(q, n_rois, L.ptr(points) if len(points) else None, len(points), L.ptr(out)), "roi_density")
    return out


def density_of(image, spacing, rois):
    """The batched call: `rois` is a list of density measures or of ``measurements.plist`` dicts (mixed freely); ONE library
    call computes all of them on `image` -- int16 (dz, dy, dx) of any strides, read from its mirror when it is bound
    (``slice_.bind_image``), or a `DeviceVolume`, whose resident image is read in place -- and the list of their results
    ``{"min", "max", "mean", "std", "area", "perimeter", "value"}`` comes back.  A measure given as an object has the values
    stored on it and on its attached measurement, as ``calc_density`` does; a dict is left alone (`recompute_measurements`
    rewrites dicts).  IndexError where the reference raises it (a slice outside the volume; np.ogrid's length quirk)."""
    measures = [measure_from_dict(r) if isinstance(r, dict) else r for r in rois]
    if hasattr(image, "roi_records"):  # a DeviceVolume
        records = image.roi_records(measures, spacing)
    else:
        q, points = describe_rois(_Grid.of(image), spacing, measures)
        L.require_device()
        records = roi_records(q, len(measures), points)
    return [m._store(stats_from_record(rec)) for m, rec in zip(measures, records)]


def recompute_measurements(project_measurements: dict, image, spacing) -> int:
    """Rewrite the density entries (type DENSITY_ELLIPSE / DENSITY_POLYGON) of a loaded ``measurements.plist`` dict in place from
    `image` -- what the reference does for its whole panel when the image changes -- in one library call; linear and angular
    entries are left alone.  Returns the number of entries rewritten."""
    keys = [k for k, info in project_measurements.items() if isinstance(info, dict) and info.get("type") in (DENSITY_ELLIPSE, DENSITY_POLYGON)]
    measures = [measure_from_dict(project_measurements[k]) for k in keys]
    density_of(image, spacing, measures)
    for k, m in zip(keys, measures):
        project_measurements[k] = m._measurement.get_as_dict()
    return len(keys)
