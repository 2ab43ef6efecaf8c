"""The 3-D mask editor: polygon cuts and 3-D brush strokes, in place on the padded mask matrix.

`Mask3DEditorState` restates the reference's class of the same name (invesalius/data/mask3d_editor_state.py) method for
method, on the kernels of csrc/k_mask3d.hip: the screen filter of all polygons is one launch, a cut is one launch on the
matrix itself, and a whole brush drag is one launch over the union of its dabs' boxes.  Its three copies of the mask --
``mask_data``, ``base_mask_data``, ``original_mask_data`` -- are device blocks.  On a matrix bound with `mask.bind_matrix`
the tool works in the mirror and only the planes that changed travel to the host; an unbound matrix is staged.

    st = Mask3DEditorState(matrix, spacing, (w, h), publish)
    st.setup_state()
    st.ReceiveVolumeViewerActiveCamera(volume.resolve_camera("iso", shape, spacing, (w, h)))
    st.insert_point(x, y, world_point) ...; st.complete_current_polygon()      # cuts
    st.SetDepthValue(0.5)                                                         # cuts again, cumulative

The module functions `polygon_filter`, `cut_mask` and `brush_stroke` are the same operations without the state.

Deviations from the reference (each also in the notes of tests/golden/ref_mask3deditor.npz):

* ``Publisher.sendMessage("M3E cut mask from 3D")`` is `publish` followed by a direct call of `CutMaskFromPolygons`: the
  state subscribes to nothing.  ``Send volume viewer size`` / ``Send volume viewer active camera`` go to `publish`, whose
  receiver may answer at once through `ReceiveVolumeViewerSize` / `ReceiveVolumeViewerActiveCamera`, as the viewer does.
* the canvas (``viewer.canvas.draw_list``, ``UpdateCanvas``), ``Slice.discard_all_buffers`` and
  ``Mask._update_imagedata`` stay with the caller: the polygons are `Polygon3D` records, and the previews read the mirror.
* `get_filters` returns the display points of every polygon; the rasters are made, ORed, transposed and inverted by one
  kernel in `CutMaskFromPolygons`.
* `brush_stroke` also takes an (N, 3) array: a whole drag, equal to N calls.
* VTK is not installed, so `camera_matrices` / `world_to_display` restate vtkCamera and vtkCoordinate for a parallel
  projection from their documentation (PARITY UNPINNED); the kernels take any 4x4 matrices."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from . import history as H
from .device import DeviceBuffer

MASK_3D_EDIT_INCLUDE = 0
MASK_3D_EDIT_EXCLUDE = 1
MASK_3D_EDIT_TOOL_POLYGON = 0
MASK_3D_EDIT_TOOL_BRUSH = 1
BRUSH_SIZE = 30


def brush_capacity() -> int:
    """centres one launch of the stroke kernel takes; a longer drag is split"""
    return int(L.lib().ivx_m3e_brush_capacity())


# ---- cameras ----------------------------------------------------------------------------------------------------------------
_INV_Y = np.diag([1.0, -1.0, 1.0, 1.0])


def _view_transform(camera) -> np.ndarray:
    """vtkCamera::GetViewTransformMatrix: rows right, up, view plane normal (focal point -> position), position to 0"""
    right, up = np.asarray(camera["right"], np.float64), np.asarray(camera["up"], np.float64)
    vpn = -np.asarray(camera["dir"], np.float64)
    pos = np.asarray(camera["position"], np.float64)
    v = np.eye(4)
    for i, axis in enumerate((right, up, vpn)):
        v[i, :3] = axis
        v[i, 3] = -float(axis @ pos)
    return v


def _projection(camera, aspect, nearz, farz, clipping_range) -> np.ndarray:
    """vtkCamera::GetProjectionTransformMatrix(aspect, nearz, farz) of a parallel projection: vtkPerspectiveTransform::Ortho
    over +-parallel_scale * aspect, +-parallel_scale and the clipping range, then AdjustZBuffer(-1, 1, nearz, farz)"""
    near, far = float(clipping_range[0]), float(clipping_range[1])
    height = float(camera["parallel_scale"])
    width = height * aspect
    p = np.eye(4)
    p[0, 0] = 2.0 / (2.0 * width)
    p[1, 1] = 2.0 / (2.0 * height)
    p[2, 2] = -2.0 / (far - near)
    p[2, 3] = -(near + far) / (far - near)
    z = np.eye(4)
    z[2, 2] = (farz - nearz) / 2.0
    z[2, 3] = (farz + nearz) / 2.0
    return z @ p


def default_clipping_range(camera):
    """a clipping range for a camera dict that carries none: (0.01 d, 2 d) for the distance d from position to focal point
    (what vtkRenderer::ResetCameraClippingRange would set depends on the scene's bounds, which a camera dict does not have)"""
    if "clipping_range" in camera:
        return tuple(float(v) for v in camera["clipping_range"])
    d = float(np.linalg.norm(np.asarray(camera["position"], np.float64) - np.asarray(camera["focal"], np.float64)))
    return (0.01 * d, 2.0 * d)


def camera_matrices(camera, size, clipping_range=None):
    """ReceiveVolumeViewerActiveCamera:135-148: (world_to_screen, world_to_camera) = (composite projection transform for
    (width / height, near, far), view transform), each multiplied by diag(1, -1, 1, 1) from the right"""
    w, h = size
    near, far = default_clipping_range(camera) if clipping_range is None else clipping_range
    mv = _view_transform(camera)
    m = _projection(camera, w / float(h), near, far, (near, far)) @ mv
    return m @ _INV_Y, mv @ _INV_Y


def world_to_display(points, camera, size, clipping_range=None) -> np.ndarray:
    """vtkCoordinate (world) .GetComputedDoubleDisplayValue(renderer) for a renderer that fills a `size` window: view
    coordinates through the composite projection transform for (aspect, -1, 1), then (v + 1) * size / 2; y runs upwards"""
    w, h = size
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    rng = default_clipping_range(camera) if clipping_range is None else clipping_range
    m = _projection(camera, w / float(h), -1.0, 1.0, rng) @ _view_transform(camera)
    out = np.empty((len(pts), 2))
    for i, p in enumerate(pts):
        v = m @ np.array([p[0], p[1], p[2], 1.0])
        out[i, 0] = (v[0] / v[3] + 1.0) * (w * 1.0) / 2.0
        out[i, 1] = (v[1] / v[3] + 1.0) * (h * 1.0) / 2.0
    return out


def display_to_world_focal_plane(display_xy, camera, size) -> np.ndarray:
    """polygon_select._display_to_world: the world point on the plane through the focal point that shows at a display point"""
    w, h = size
    xy = np.asarray(display_xy, np.float64).reshape(-1, 2)
    height = float(camera["parallel_scale"])
    width = height * (w / float(h))
    right, up = np.asarray(camera["right"], np.float64), np.asarray(camera["up"], np.float64)
    focal, pos = np.asarray(camera["focal"], np.float64), np.asarray(camera["position"], np.float64)
    vx = xy[:, 0] * 2.0 / w - 1.0
    vy = xy[:, 1] * 2.0 / h - 1.0
    # the focal point's own view coordinates (0 for a camera that looks at it)
    fx, fy = float(right @ (focal - pos)) / width, float(up @ (focal - pos)) / height
    return focal + np.outer((vx - fx) * width, right) + np.outer((vy - fy) * height, up)


# ---- the operations ---------------------------------------------------------------------------------------------------------
def _mode(edit_mode) -> int:
    return int(edit_mode)


def _pack_polygons(polygons):
    """K polygons of display points -> ((P, 2) float64 points, K + 1 int64 offsets)"""
    polys = []
    for p in polygons:
        a = np.asarray(p, np.float64)
        if a.size == 0:
            a = np.zeros((0, 2))
        if a.ndim != 2 or a.shape[1] < 2:
            raise TypeError("a polygon is an (N, 2) array of display points")
        polys.append(np.ascontiguousarray(a[:, :2]))
    offsets = np.zeros(len(polys) + 1, np.int64)
    if polys:
        offsets[1:] = np.cumsum([len(p) for p in polys])
    points = np.concatenate(polys) if polys else np.zeros((0, 2))
    return np.ascontiguousarray(points, np.float64), offsets


def _filter_mode(edit_mode) -> int:
    m = _mode(edit_mode)
    if m not in (MASK_3D_EDIT_INCLUDE, MASK_3D_EDIT_EXCLUDE):
        raise ValueError("edit mode %r: MASK_3D_EDIT_INCLUDE or MASK_3D_EDIT_EXCLUDE" % (edit_mode,))
    return m


def polygon_filter(size, polygons, edit_mode) -> np.ndarray:
    """The screen filter of CutMaskFromPolygons:196-200 as an (h, w) bool array:
    ``np.logical_or.reduce([polygon2mask_rs((w, h), p) for p in polygons]).T``, inverted for MASK_3D_EDIT_INCLUDE; no polygon
    gives all False (all True).  One launch, whatever the number of polygons."""
    w, h = int(size[0]), int(size[1])
    if w < 0 or h < 0:
        raise OverflowError("size must be non-negative")
    mode = _filter_mode(edit_mode)
    points, offsets = _pack_polygons(polygons)
    out = np.zeros((h, w), np.uint8)
    L.check(L.lib().ivx_m3e_filter(w, h, L.ptr(points), L.ptr(offsets), len(offsets) - 1, mode, L.ptr(out)), "polygon_filter")
    return out.view(np.bool_)


def _padded(mask_matrix, what):
    m = mask_matrix
    if not isinstance(m, np.ndarray) or m.dtype != np.uint8 or m.ndim != 3 or not m.flags["C_CONTIGUOUS"]:
        raise TypeError("%s: the padded mask matrix, a C-contiguous 3-D uint8 array" % what)
    if min(m.shape) < 1:
        raise TypeError("%s: the padded mask matrix has at least one plane along every axis" % what)
    if not m.flags.writeable:
        raise TypeError("%s: the mask matrix must be writable" % what)
    return m, L.i64([s - 1 for s in m.shape]), L.i64(m.strides)


def _mat4(a, name):
    a = np.ascontiguousarray(a, np.float64)
    if a.shape != (4, 4):
        raise ValueError("%s must be 4x4" % name)
    return a


def _d3(v):
    return (ctypes.c_double * 3)(*[float(x) for x in v])


def cut_mask(mask_matrix, spacing, filter_or_polygons, size, m, mv, depth, edit_mode) -> int:
    """mask_cut on ``mask_matrix[1:, 1:, 1:]`` in place.  `filter_or_polygons`: the (h, w) bool filter (`polygon_filter`), or
    the polygons' display points, from which the filter is made on the device; `size` = (w, h); `m` / `mv` world -> screen and
    world -> camera; `depth` the greatest distance from the camera that is cut.  Returns the planes written on the host."""
    mat, shape, strides = _padded(mask_matrix, "cut_mask")
    w, h = int(size[0]), int(size[1])
    m, mv = _mat4(m, "m"), _mat4(mv, "mv")
    mode = _mode(edit_mode)
    written = L.c_i64(0)
    lib = L.lib()
    if isinstance(filter_or_polygons, np.ndarray) and filter_or_polygons.dtype in (np.bool_, np.uint8) and filter_or_polygons.ndim == 2:
        f = np.ascontiguousarray(filter_or_polygons).view(np.uint8)
        if f.shape != (h, w):
            raise ValueError("cut_mask: the filter has shape %r, the viewport is %r" % (f.shape, (h, w)))
        L.check(lib.ivx_m3e_cut(L.ptr(mat), shape, strides, _d3(spacing), float(depth), L.ptr(f), h, w, None, None, 0, L.ptr(m), L.ptr(mv),
                                mode, ctypes.byref(written)), "cut_mask")
    else:
        points, offsets = _pack_polygons(filter_or_polygons)
        L.check(lib.ivx_m3e_cut(L.ptr(mat), shape, strides, _d3(spacing), float(depth), None, h, w, L.ptr(points), L.ptr(offsets),
                                len(offsets) - 1, L.ptr(m), L.ptr(mv), _filter_mode(mode), ctypes.byref(written)), "cut_mask")
    return int(written.value)


def brush_centres(world_coords, spacing) -> np.ndarray:
    """brush_stroke:239-250: ``(wx + sx, -wy - sy, wz + sz)`` for every world point.  (The reference's centre is in the
    coordinates of the padded matrix while the kernel indexes the interior: kept as it is.)"""
    wc = np.asarray(world_coords, np.float64).reshape(-1, 3)
    sx, sy, sz = (float(v) for v in spacing)
    c = np.empty_like(wc)
    c[:, 0] = wc[:, 0] + sx
    c[:, 1] = -wc[:, 1] - sy
    c[:, 2] = wc[:, 2] + sz
    return np.ascontiguousarray(c)


def brush_stroke(mask_matrix, orig_matrix, spacing, world_coords, brush_size, edit_mode) -> int:
    """A drag of the 3-D brush on ``mask_matrix[1:, 1:, 1:]`` in place: one dab of brush_mask_rs per world point, radius
    ``brush_size / 2``.  `orig_matrix`: the padded matrix that include mode reveals, or None (255 is painted).  Returns the
    planes written on the host."""
    mat, shape, strides = _padded(mask_matrix, "brush_stroke")
    orig = None
    if orig_matrix is not None:
        orig, _, _ = _padded(orig_matrix, "brush_stroke (orig)")
        if orig.shape != mat.shape:
            raise IndexError("orig and the mask matrix differ in shape")
    centres = brush_centres(world_coords, spacing)
    written = L.c_i64(0)
    L.check(L.lib().ivx_m3e_brush_stroke(L.ptr(mat), L.ptr(orig) if orig is not None else None, shape, strides, _d3(spacing), L.ptr(centres),
                                         len(centres), float(brush_size) / 2.0, _mode(edit_mode), ctypes.byref(written)), "brush_stroke")
    return int(written.value)


# ---- the state machine ------------------------------------------------------------------------------------------------------
class Polygon3D:
    """what the state machine uses of PolygonSelectCanvas (polygon_select.py:44-136): the world points, the display points
    as they were clicked, `complete`"""

    def __init__(self):
        self.points = []
        self._world_points = []
        self.complete = False
        self.visible = True
        self.interactive = True

    def insert_point(self, display_point, world_point):
        self.points.append(tuple(display_point))
        self._world_points.append(tuple(world_point))

    def complete_polygon(self):
        if len(self.points) >= 3:
            self.complete = True

    def set_interactive(self, value):
        self.interactive = bool(value)


class Mask3DEditorState:
    """Mask3DEditorState of the reference on device blocks.  `mask_matrix`: the current mask's padded matrix (bound or not),
    or None for "no mask"; `spacing` (sx, sy, sz); `size` the viewport (w, h); `publish(topic, **kw)` receives the messages.
    `history`: the mask's `history.EditionHistory` (a stroke records a VOLUME node there); `mask_3d_preview`: the session's
    flag, read by `setup_state`."""

    def __init__(self, mask_matrix, spacing, size, publish=None, history=None, mask_3d_preview=False):
        self.matrix = None
        self.set_mask(mask_matrix)
        self.spacing = tuple(float(v) for v in spacing)
        self.resolution = (int(size[0]), int(size[1]))
        self._publish = publish
        self.history = history
        self.mask_3d_preview = bool(mask_3d_preview)
        self.mask_data = None
        self.base_mask_data = None
        self.m3e_list = []
        self.edit_mode = MASK_3D_EDIT_EXCLUDE
        self.tool_mode = MASK_3D_EDIT_TOOL_POLYGON
        self.brush_size = float(BRUSH_SIZE)
        self.depth_val = 1.0
        self.has_set_mask_preview = False
        self.has_cleared_for_crop = False
        self.world_to_screen = None
        self.world_to_camera_coordinates = None
        self.clipping_range = None
        self.camera = None
        self.was_edited = False
        self.planes_written = 0  # by the last update_views

    # -- plumbing
    def set_mask(self, mask_matrix):
        """``Slice().current_mask`` changed hands (None: no mask); follow with `OnMaskChanged`"""
        if mask_matrix is not None:
            _padded(mask_matrix, "Mask3DEditorState")
        self.matrix = mask_matrix

    def _send(self, topic, **kw):
        if self._publish is not None:
            self._publish(topic, **kw)

    def _geometry(self):
        return L.i64([s - 1 for s in self.matrix.shape]), L.i64(self.matrix.strides)

    def _matrix_copy(self) -> DeviceBuffer:
        """``cur_mask.matrix.copy()`` as a device block; a bound matrix is read from its mirror"""
        b = H._Block(self.matrix.nbytes)
        try:
            b.upload_view(self.matrix)
        except Exception:
            b.close()
            raise
        return b

    def _set(self, name, block):
        old = getattr(self, name, None)
        if old is not None and old is not block:
            old.close()
        setattr(self, name, block)

    def _flags(self) -> DeviceBuffer:
        n = self.matrix.shape[0]
        f = getattr(self, "_plane_flags", None)
        if f is None or f.nbytes < n:
            if f is not None:
                f.close()
            f = self._plane_flags = DeviceBuffer(n)
        f.zero()
        return f

    def download(self, name="mask_data") -> np.ndarray:
        """a host copy of one of the device blocks, for inspection"""
        b = getattr(self, name)
        return b.download(self.matrix.shape, np.uint8)

    def close(self):
        for name in ("mask_data", "base_mask_data", "original_mask_data", "_plane_flags"):
            b = getattr(self, name, None)
            if b is not None:
                b.close()
                setattr(self, name, None)

    # -- the reference's methods
    def setup_state(self):
        self._send("M3E ask for edit mode")
        self._send("M3E ask for tool mode")
        self._send("M3E ask for depth value")
        if not self.mask_3d_preview:
            self.has_set_mask_preview = True
            self._send("Enable mask 3D preview")
        if self.matrix is not None:
            self._set("mask_data", self._matrix_copy())
        if not self.has_set_mask_preview:
            self._send("Render volume viewer")

    def cleanup_state(self):
        self.m3e_list.clear()
        if self.has_set_mask_preview:
            self._send("Disable mask 3D preview")

    def _cut_message(self):
        self._send("M3E cut mask from 3D")
        self.CutMaskFromPolygons()

    def SetEditMode(self, mode):
        self.edit_mode = mode
        self.has_cleared_for_crop = False
        self._cut_message()

    def SetToolMode(self, tool):
        self.tool_mode = tool

    def SetDepthValue(self, value):
        self.depth_val = value
        self._cut_message()

    def SetBrushSize(self, size):
        self.brush_size = size

    def init_new_polygon(self):
        self.m3e_list.append(Polygon3D())

    def insert_point(self, mouse_x, mouse_y, world_point):
        if len(self.m3e_list) == 0 or self.m3e_list[-1].complete:
            self.init_new_polygon()
        self.m3e_list[-1].insert_point((mouse_x, mouse_y), world_point)

    def complete_current_polygon(self):
        if len(self.m3e_list) > 0 and not self.m3e_list[-1].complete:
            self.m3e_list[-1].complete_polygon()
            self._cut_message()

    def ClearPolygons(self):
        self.m3e_list.clear()
        self.OnRestoreInitMask()

    def ReceiveVolumeViewerActiveCamera(self, cam):
        """`cam`: a camera dict of `volume.resolve_camera` (with ``clipping_range``, or `default_clipping_range`), or
        ``(m, mv, clipping_range)`` with the two matrices as the reference stores them"""
        if isinstance(cam, dict):
            self.camera = cam
            self.clipping_range = default_clipping_range(cam)
            self.world_to_screen, self.world_to_camera_coordinates = camera_matrices(cam, self.resolution, self.clipping_range)
        else:
            m, mv, rng = cam
            self.camera = None
            self.clipping_range = (float(rng[0]), float(rng[1]))
            self.world_to_screen, self.world_to_camera_coordinates = _mat4(m, "m"), _mat4(mv, "mv")

    def ReceiveVolumeViewerSize(self, size):
        self.resolution = (int(size[0]), int(size[1]))

    def OnRestoreInitMask(self):
        if self.mask_data is not None:
            self.update_views()

    def display_points(self, world_points) -> np.ndarray:
        """vtkCoordinate.GetComputedDoubleDisplayValue for the camera last received; a state that was given matrices instead
        of a camera dict needs `to_display` set by the caller"""
        to_display = getattr(self, "to_display", None)
        if to_display is not None:
            return np.asarray(to_display(world_points), np.float64).reshape(-1, 2)
        if self.camera is None:
            raise RuntimeError("Mask3DEditorState: no camera dict received and no to_display set")
        return world_to_display(world_points, self.camera, self.resolution, self.clipping_range)

    def get_filters(self):
        """the display points of every polygon of the list, complete or not (the reference rasterises each here; the raster
        of all of them is one launch in CutMaskFromPolygons)"""
        out = []
        for poly in self.m3e_list:
            out.append(self.display_points(poly._world_points) if poly._world_points else np.zeros((0, 2)))
        return out

    def CutMaskFromPolygons(self):
        completed = [p for p in self.m3e_list if p.complete]
        if len(completed) == 0:
            return
        if self.mask_data is None:
            return
        self._send("Send volume viewer size")
        self._send("Send volume viewer active camera")
        w, h = self.resolution
        if h == 0:
            return
        polygons = self.get_filters()
        if self.clipping_range is None or self.world_to_screen is None or self.world_to_camera_coordinates is None:
            return
        near, far = self.clipping_range
        depth = near + (far - near) * self.depth_val
        mode = _filter_mode(self.edit_mode)
        lib = L.lib()
        points, offsets = _pack_polygons(polygons)
        blk = DeviceBuffer(points.nbytes + offsets.nbytes + 16 + h * w)
        try:
            # offsets, points, filter in one block (8-byte items first)
            blk.upload(np.concatenate([offsets.view(np.uint8), points.reshape(-1).view(np.uint8)]))
            d_off, d_pts, d_f = blk.at(0), blk.at(offsets.nbytes), blk.at(offsets.nbytes + points.nbytes)
            L.check(lib.ivx_dev_m3e_filter(w, h, d_pts, d_off, len(offsets) - 1, mode, d_f, None), "CutMaskFromPolygons")
            shape, strides = self._geometry()
            m, mv = _mat4(self.world_to_screen, "m"), _mat4(self.world_to_camera_coordinates, "mv")
            L.check(lib.ivx_dev_m3e_cut(self.mask_data.ptr, shape, strides, _d3(self.spacing), float(depth), d_f, h, w, L.ptr(m), L.ptr(mv),
                                        mode, self._flags().ptr, None), "CutMaskFromPolygons")
            L.synchronize()
        finally:
            blk.close()
        self.update_views()

    def brush_stroke(self, world_coord):
        if self.mask_data is None:
            return
        w, h = self.resolution
        if h == 0:
            return
        centres = brush_centres(world_coord, self.spacing)
        orig = None
        if self.edit_mode == 0 and self.base_mask_data is not None:
            orig = self.base_mask_data
        elif getattr(self, "original_mask_data", None) is not None:
            orig = self.original_mask_data
        d_c = DeviceBuffer(max(centres.nbytes, 16))
        try:
            d_c.upload(centres)
            shape, strides = self._geometry()
            L.check(L.lib().ivx_dev_m3e_brush_stroke(self.mask_data.ptr, orig.ptr if orig is not None else None, shape, strides,
                                                     _d3(self.spacing), L.ptr(centres), d_c.ptr, len(centres), float(self.brush_size) / 2.0,
                                                     int(self.edit_mode), self._flags().ptr, None), "brush_stroke")
            L.synchronize()
        finally:
            d_c.close()
        self.update_views()

    def OnMaskChanged(self, index=0):
        if self.matrix is not None:
            self._set("mask_data", self._matrix_copy())
            self.has_cleared_for_crop = False

    def update_views(self, _mat=None):
        """``cur_mask.matrix[1:, 1:, 1:] = mask_data[1:, 1:, 1:]``, host and mirror: the bytes that differ are stored and the
        planes that hold one are copied to the host"""
        if self.matrix is not None:
            shape, strides = self._geometry()
            written = L.c_i64(0)
            L.check(L.lib().ivx_m3e_apply(L.ptr(self.matrix), self.mask_data.ptr, shape, strides, ctypes.byref(written)), "update_views")
            self.planes_written = int(written.value)
            self.was_edited = True
        self._send("Reload actual slice")
        self._send("Update slice viewer")

    def start_brush_stroke(self):
        if self.matrix is None:
            return
        self._set("mask_data", self._matrix_copy())
        self._set("original_mask_data", self._matrix_copy())
        if self.edit_mode == 0:
            same = False
            if self.has_cleared_for_crop and self.base_mask_data is not None:
                eq = ctypes.c_int(0)
                L.check(L.lib().ivx_dev_m3e_equal(self.mask_data.ptr, self.base_mask_data.ptr, self.matrix.nbytes, ctypes.byref(eq), None),
                        "start_brush_stroke")
                same = bool(eq.value)
            if not self.has_cleared_for_crop or same:
                self._set("base_mask_data", self._matrix_copy())
                self.mask_data.zero(nbytes=self.matrix.nbytes)
                self.has_cleared_for_crop = True

    def end_brush_stroke(self):
        if self.matrix is None:
            return
        n, shape = self.matrix.nbytes, self.matrix.shape
        if self.history is not None:
            # mask.save_history(0, "VOLUME", self.original_mask_data, self.mask_data): array, p_array in the reference's order
            array = H.snapshot_device(self.original_mask_data.ptr, n, shape)
            try:
                p_array = H.snapshot_device(self.mask_data.ptr, n, shape)
            except Exception:
                array.close()
                raise
            self.history.new_node(0, H.VOLUME, array, p_array, False)
        self._set("mask_data", self._matrix_copy())
        self._modified_all_volume()

    def _modified_all_volume(self):
        """Mask.modified(all_volume=True): the three flag planes become 1, on the host and in the mirror"""
        shape, strides = self._geometry()
        L.check(L.lib().ivx_m3e_flag_planes(L.ptr(self.matrix), shape, strides), "end_brush_stroke")
