"""The surface view: shaded pictures of surfaces on the GPU (csrc/k_surfview.hip).

The reference shows a surface by putting its polydata behind a vtkPolyDataMapper and a vtkActor with back-face culling, a
colour, an opacity of ``1 - transparency`` and the session's interpolation mode (Surface._show_surface,
invesalius/data/surface.py:1061-1116), under the parallel-projection camera of the 3-D viewer, and writes the view to a file
with viewer_volume.OnExportPicture.  Here that is a software rasteriser whose picture is a function of its input alone: an
id-and-depth pass that keeps, per pixel and surface, the 64-bit minimum of (ordered depth, triangle index), and a resolve
pass that shades the winners (flat, Gouraud or Phong under one white headlight) and blends up to eight surfaces, sorted by
depth, over the background.  The camera is `volume.camera_for_view`'s dict, so a surface picture lines up pixel for pixel
with `DeviceVolume.render_volume` and `render_mask_preview` of the same case.

PARITY UNPINNED vs VTK's OpenGL renderer (not installed): the rules of DESIGN 7n are the contract; they are pinned against
the numpy restatement tests/_surface_view_ref.py.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from . import volume as V

# the reference's defaults (constants.py:317-334, 370; session.py:48), compared with tests/golden/ref_surfaceview.json
SURFACE_TRANSPARENCY = 0.0
SURFACE_INTERPOLATION = 1
SURFACE_COLOUR = [
    (0.33, 1, 0.33), (1, 1, 0.33), (0.33, 0.91, 1), (1, 0.33, 1), (1, 0.68, 0.33), (1, 0.33, 0.33),
    (0.33333333333333331, 0.33333333333333331, 1.0), (1.0, 0.33333333333333331, 0.66666666666666663),
    (0.74901960784313726, 1.0, 0.0), (0.83529411764705885, 0.33333333333333331, 1.0),
    (0.792156862745098, 0.66666666666666663, 1.0), (1.0, 0.66666666666666663, 0.792156862745098),
    (0.33333333333333331, 1.0, 0.83529411764705885), (1.0, 0.792156862745098, 0.66666666666666663),
    (0.792156862745098, 1.0, 0.66666666666666663), (0.66666666666666663, 0.792156862745098, 1.0),
]
INTERPOLATIONS = {"flat": 0, "gouraud": 1, "phong": 2}
MAX_SURFACES = 8
RASTER_CLEAR, RASTER_SMALL, RASTER_BIG, RASTER_ALL = 1, 2, 4, 7
c64 = ctypes.c_int64


class SurfaceCamera(ctypes.Structure):
    """struct ivx_surface_camera (include/ivx.h)."""
    _fields_ = [("focal", ctypes.c_double * 3), ("right", ctypes.c_double * 3), ("up", ctypes.c_double * 3),
                ("dir", ctypes.c_double * 3), ("parallel_scale", ctypes.c_double), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32)]


class SurfaceLayer(ctypes.Structure):
    """struct ivx_surface_layer (include/ivx.h)."""
    _fields_ = [("verts", ctypes.c_void_p), ("nverts", c64), ("faces", ctypes.c_void_p), ("ntris", c64),
                ("normals", ctypes.c_void_p), ("keys", ctypes.c_void_p), ("rgb", ctypes.c_float * 3), ("opacity", ctypes.c_float)]


def camera_for_bounds(view: str, bounds6, viewport) -> dict:
    """`volume.camera_for_view` for a scene without an image: what it does after `volume_bounds`, from the bounds
    (xmin, xmax, ymin, ymax, zmin, zmax) themselves"""
    return V.camera_from_bounds(view, tuple(float(x) for x in bounds6), viewport)


def _resolve_camera(camera, size, shape, spacing, bounds) -> dict:
    """A camera dict as it is; a standard view name as the camera of the image `shape` when given, else of `bounds()`; either
    way with the viewport `size` (width, height)."""
    viewport = (int(size[0]), int(size[1]))
    if viewport[0] <= 0 or viewport[1] <= 0:
        raise ValueError("size %r must be positive" % (size,))
    if not isinstance(camera, str):
        return dict(camera, viewport=viewport)
    if shape is not None:
        return V.camera_for_view(camera, shape, (1.0, 1.0, 1.0) if spacing is None else spacing, viewport)
    return camera_for_bounds(camera, bounds(), viewport)


def _merge_bounds(bs) -> tuple:
    bs = list(bs)
    return (0.0,) * 6 if not bs else tuple(f(b[q] for b in bs) for q, f in enumerate((min, max) * 3))


def _c_camera(cam: dict) -> SurfaceCamera:
    c = SurfaceCamera()
    c.focal[:], c.right[:], c.up[:], c.dir[:] = ([float(x) for x in cam[k]] for k in ("focal", "right", "up", "dir"))
    c.parallel_scale = float(cam["parallel_scale"])
    c.width, c.height = (int(x) for x in cam["viewport"])
    return c


def _interpolation(mode) -> int:
    if isinstance(mode, str):
        if mode.lower() not in INTERPOLATIONS:
            raise ValueError("unknown interpolation %r (one of %s)" % (mode, ", ".join(INTERPOLATIONS)))
        return INTERPOLATIONS[mode.lower()]
    if int(mode) not in (0, 1, 2):
        raise ValueError("interpolation %r is not 0 (flat), 1 (Gouraud) or 2 (Phong)" % (mode,))
    return int(mode)


class SurfaceActor:
    """One surface of a scene: a mesh (host arrays, or a `polydata_utils.DeviceMesh` with an optional device buffer of one
    float32 normal per point), its colour, transparency and visibility -- what the reference keeps on the vtkActor."""

    def __init__(self, verts, faces=None, normals=None, colour=SURFACE_COLOUR[0], transparency=SURFACE_TRANSPARENCY, visible=True):
        from .polydata_utils import DeviceMesh
        self.mesh = verts if isinstance(verts, DeviceMesh) else None
        if self.mesh is None:
            self.verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
            self.faces = np.ascontiguousarray(np.zeros((0, 3), np.int32) if faces is None else faces, np.int32).reshape(-1, 3)
            if len(self.faces) and (self.faces.min() < 0 or self.faces.max() >= len(self.verts)):
                raise ValueError("surface: face index outside [0, %d)" % len(self.verts))
            self.normals = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            if self.normals is not None and len(self.normals) != len(self.verts):
                raise ValueError("surface: %d normals for %d points" % (len(self.normals), len(self.verts)))
        else:
            self.verts = self.faces = None
            self.normals = normals  # a DeviceBuffer, or None
        self.colour = colour
        self.transparency = transparency
        self.visible = bool(visible)

    @property
    def colour(self):
        return self._colour

    @colour.setter
    def colour(self, c):
        c = tuple(float(x) for x in c)
        if len(c) != 3 or not all(0.0 <= x <= 1.0 for x in c):
            raise ValueError("surface colour %r: three numbers in 0..1" % (c,))
        self._colour = c

    @property
    def transparency(self):
        return self._transparency

    @transparency.setter
    def transparency(self, t):
        if not 0.0 <= float(t) <= 1.0:
            raise ValueError("surface transparency %r must lie in 0..1" % (t,))
        self._transparency = float(t)


class _Resident:
    """an actor's mesh on the device, its key buffer and what the keys were made for"""

    def __init__(self, actor: SurfaceActor, stream):
        from .device import DeviceBuffer
        from .polydata_utils import DeviceMesh
        self.actor = actor
        self.owned = actor.mesh is None
        if self.owned:
            self.mesh = DeviceMesh.upload(actor.verts, actor.faces, stream)
            self.normals = None
            if actor.normals is not None:
                self.normals = DeviceBuffer(actor.normals.nbytes + 16)
                if len(actor.normals):
                    self.normals.upload(actor.normals)
        else:
            self.mesh, self.normals = actor.mesh, actor.normals
        self.keys = None
        self.keys_for = None  # (camera bytes, nverts, ntris) of the last raster

    def close(self):
        if self.owned:
            self.mesh.close()
            if self.normals is not None:
                self.normals.close()
        if self.keys is not None:
            self.keys.close()
        self.keys = None


class Scene:
    """The actor list of one 3-D view.  Meshes given as host arrays are uploaded once; the key buffer of every surface is kept
    across calls, so a render after a change of colour, transparency, interpolation or background runs the resolve alone
    (`raster_runs` counts the raster calls, `last_stages` holds the stage bits of the last render per visible surface).  A
    change of camera, size or visibility of a surface rasterises again what it must.  `invalidate()` after the points of a
    resident mesh were changed in place."""

    def __init__(self, actors=(), stream=None):
        self.stream = stream
        self._res = []
        self.raster_runs = 0
        self.last_stages = []
        self._out = {}       # name -> DeviceBuffer of the picture, the ids, the depth
        self._last = None    # (camera dict, visible residents) of the last render, for pick
        for a in actors:
            self.add(a)

    def add(self, actor: SurfaceActor) -> SurfaceActor:
        self._res.append(_Resident(actor, self.stream))
        return actor

    @property
    def actors(self):
        return [r.actor for r in self._res]

    def invalidate(self):
        for r in self._res:
            r.keys_for = None

    def _sync(self):
        L.check(L.lib().ivx_stream_synchronize(self.stream) if self.stream else L.lib().ivx_device_synchronize())

    def bounds(self):
        """the bounds of the visible surfaces' points: ivx_dev_mesh_bounds per surface, merged on the host"""
        return _merge_bounds(r.mesh.bounds() for r in self._res if r.actor.visible and r.mesh.nverts)

    def camera(self, camera="iso", size=(512, 512), shape=None, spacing=None) -> dict:
        return _resolve_camera(camera, size, shape, spacing, self.bounds)

    def _buffer(self, name, nbytes):
        from .device import DeviceBuffer
        have = self._out.get(name)
        if have is None or have.nbytes < nbytes:
            if have is not None:
                have.close()
            have = self._out[name] = DeviceBuffer(nbytes)
        return have

    def raster(self, cam: dict):
        """The key buffers of the visible surfaces for the camera dict `cam`, rastered where they are not already those of
        this camera and mesh: (the C camera, the visible residents, the `SurfaceLayer` table with mesh, keys, colour and
        opacity filled in).  What `render` and `scene3d.Scene3D.render` resolve."""
        lib = L.lib()
        visible = [r for r in self._res if r.actor.visible]
        if len(visible) > MAX_SURFACES:
            raise TypeError("surface view: %d visible surfaces (at most %d)" % (len(visible), MAX_SURFACES))
        cc = _c_camera(cam)
        npix = cc.width * cc.height
        layers = (SurfaceLayer * MAX_SURFACES)()
        self.last_stages = []
        for k, r in enumerate(visible):
            made_for = (bytes(cc), r.mesh.nverts, r.mesh.ntris, r.mesh.verts.ptr.value, r.mesh.faces.ptr.value)
            stages = 0
            if r.keys is None or r.keys.nbytes < npix * 8 or r.keys_for != made_for:
                from .device import DeviceBuffer
                if r.keys is None or r.keys.nbytes < npix * 8:
                    if r.keys is not None:
                        r.keys.close()
                    r.keys = DeviceBuffer(npix * 8)
                stages = RASTER_ALL
                L.check(lib.ivx_dev_surface_raster(r.mesh.verts.ptr, c64(r.mesh.nverts), r.mesh.faces.ptr, c64(r.mesh.ntris),
                                                   ctypes.byref(cc), stages, r.keys.ptr, self.stream), "surface_raster")
                r.keys_for = made_for
                self.raster_runs += 1
            self.last_stages.append(stages)
            m = layers[k]
            m.verts, m.nverts, m.faces, m.ntris = r.mesh.verts.ptr, r.mesh.nverts, r.mesh.faces.ptr, r.mesh.ntris
            m.normals = r.normals.ptr if r.normals is not None else None
            m.keys = r.keys.ptr
            m.rgb[:] = r.actor.colour
            m.opacity = 1.0 - r.actor.transparency
        return cc, visible, layers

    def render(self, camera="iso", size=(512, 512), shape=None, spacing=None, interpolation=SURFACE_INTERPOLATION,
               background=(0.0, 0.0, 0.0), rgba8=False, depth=False, ids=False, download=True):
        """The picture: float32 RGBA (H, W, 4), or uint8 with `rgba8`; with `depth` and / or `ids` a dict that also holds the
        nearest fragment's float32 depth along the view direction (+inf where empty) and its int32 (surface, triangle) (-1
        where empty; `surface` counts the VISIBLE actors in order).  With ``download=False`` the device buffers are returned
        instead of arrays (they belong to the scene and are overwritten by its next render)."""
        lib = L.lib()
        mode = _interpolation(interpolation)
        cam = self.camera(camera, size, shape, spacing)
        cc, visible, layers = self.raster(cam)
        w, h = cc.width, cc.height
        npix = w * h
        pic = self._buffer("rgba8" if rgba8 else "rgba", npix * (4 if rgba8 else 16))
        d_ids, d_depth = self._buffer("ids", npix * 8), self._buffer("depth", npix * 4)  # always: pick reads them
        bg = (ctypes.c_float * 3)(*[float(x) for x in background])
        L.check(lib.ivx_dev_surface_resolve(layers, len(visible), ctypes.byref(cc), mode, bg, int(bool(rgba8)), pic.ptr, d_ids.ptr,
                                            d_depth.ptr, self.stream), "surface_resolve")
        self._last = (cam, visible)
        if not download:
            return {"rgba": pic, "depth": d_depth, "ids": d_ids}
        self._sync()
        out = {"rgba": pic.download((h, w, 4), np.uint8 if rgba8 else np.float32)}
        if depth:
            out["depth"] = d_depth.download((h, w), np.float32)
        if ids:
            out["ids"] = d_ids.download((h, w, 2), np.int32)
        return out if (depth or ids) else out["rgba"]

    def download_keys(self, surface: int = 0) -> np.ndarray:
        """the uint64 key buffer (H, W) of the last render's visible surface `surface`: (ordered depth << 32) | triangle"""
        if self._last is None:
            raise RuntimeError("Scene.download_keys: nothing has been rendered")
        cam, visible = self._last
        w, h = cam["viewport"]
        self._sync()
        return visible[surface].keys.download((h, w), np.uint64)

    def pick(self, col: int, row: int):
        """What lies under the centre of pixel (col, row) of the last render: None for the background, else a dict with the
        `surface` (index among the visible actors), the `triangle`, the world `position` (the pixel centre of
        `volume.pixel_rays` plus depth x dir) and `point_id`, the id of the nearest of the triangle's three corners -- the id
        `JoinSeedsParts` and the geodesic measure take.  Reads 60 bytes from the device, not the buffers."""
        if self._last is None:
            raise RuntimeError("Scene.pick: nothing has been rendered")
        cam, visible = self._last
        w, h = cam["viewport"]
        col, row = int(col), int(row)
        if not (0 <= col < w and 0 <= row < h):
            raise IndexError("pixel (%d, %d) outside %d x %d" % (col, row, w, h))
        self._sync()
        pix = row * w + col
        s, tri = (int(x) for x in _read(self._out["ids"], pix * 8, (2,), np.int32))
        if s < 0:
            return None
        t = float(_read(self._out["depth"], pix * 4, (1,), np.float32)[0])
        mesh = visible[s].mesh
        corners = _read(mesh.faces, tri * 12, (3,), np.int32)
        pts = np.stack([_read(mesh.verts, int(c) * 12, (3,), np.float32) for c in corners]).astype(np.float64)
        origin, du, dv = V.pixel_rays(dict(cam, **{k: np.asarray(cam[k], np.float64) for k in ("focal", "right", "up")}))
        pos = origin + du * col + dv * row + t * np.asarray(cam["dir"], np.float64)
        near = int(np.argmin(((pts - pos) ** 2).sum(axis=1)))
        return {"surface": s, "actor": visible[s].actor, "triangle": tri, "position": pos, "point_id": int(corners[near]), "depth": t}

    def close(self):
        for r in self._res:
            r.close()
        for b in self._out.values():
            b.close()
        self._res, self._out, self._last = [], {}, None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _read(buf, offset: int, shape, dtype) -> np.ndarray:
    """a few bytes of a device buffer, from `offset`"""
    out = np.empty(shape, dtype)
    L.check(L.lib().ivx_memcpy_d2h(L.ptr(out), buf.at(offset), ctypes.c_size_t(out.nbytes)))
    return out


def render_surfaces(actors, camera="iso", size=(512, 512), shape=None, spacing=None, interpolation=SURFACE_INTERPOLATION,
                    background=(0.0, 0.0, 0.0), rgba8=False, depth=False, ids=False, download=True):
    """One picture of `actors` (`SurfaceActor`s; the invisible ones are left out).  `camera`: a standard view name -- of the
    image when its `shape` (and `spacing`) are given, so that the picture overlays `render_volume`, else of the scene's own
    bounds -- or a camera dict.  See `Scene.render` for the result.

    Actors made of host arrays alone go through the host form (`ivx_surface_render`: upload, raster, resolve, download in one
    call); a scene that holds a resident mesh, or ``download=False``, goes through a `Scene`, which is returned along with the
    buffers for the caller to close."""
    actors = list(actors)
    if download and all(a.mesh is None for a in actors):
        return _render_host(actors, camera, size, shape, spacing, interpolation, background, rgba8, depth, ids)
    scene = Scene(actors)
    try:
        out = scene.render(camera, size, shape, spacing, interpolation, background, rgba8, depth, ids, download)
    except BaseException:
        scene.close()
        raise
    if download:
        scene.close()
        return out
    return dict(out, scene=scene)


def _render_host(actors, camera, size, shape, spacing, interpolation, background, rgba8, depth, ids):
    mode = _interpolation(interpolation)
    visible = [a for a in actors if a.visible]
    if len(visible) > MAX_SURFACES:
        raise TypeError("surface view: %d visible surfaces (at most %d)" % (len(visible), MAX_SURFACES))
    from . import polydata_utils as pu
    cam = _resolve_camera(camera, size, shape, spacing, lambda: _merge_bounds(pu.bounds(a.verts) for a in visible if len(a.verts)))
    cc = _c_camera(cam)
    w, h = cam["viewport"]
    layers = (SurfaceLayer * MAX_SURFACES)()
    for m, a in zip(layers, visible):
        m.verts, m.nverts, m.faces, m.ntris = a.verts.ctypes.data, len(a.verts), a.faces.ctypes.data, len(a.faces)
        m.normals = a.normals.ctypes.data if a.normals is not None else None
        m.rgb[:] = a.colour
        m.opacity = 1.0 - a.transparency
    out = {"rgba": np.empty((h, w, 4), np.uint8 if rgba8 else np.float32)}
    if depth:
        out["depth"] = np.empty((h, w), np.float32)
    if ids:
        out["ids"] = np.empty((h, w, 2), np.int32)
    bg = (ctypes.c_float * 3)(*[float(x) for x in background])
    L.check(L.lib().ivx_surface_render(layers, len(visible), ctypes.byref(cc), mode, bg, int(bool(rgba8)), L.ptr(out["rgba"]),
                                       L.ptr(out["ids"]) if ids else None, L.ptr(out["depth"]) if depth else None), "surface_render")
    return out if (depth or ids) else out["rgba"]
