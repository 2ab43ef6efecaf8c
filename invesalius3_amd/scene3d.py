"""The 3-D scene: the ray-cast volume, the surfaces and the three slice planes in one picture (csrc/k_scene3d.hip).

The reference's 3-D viewer holds four kinds of object in one vtkRenderer -- the surface actors, the ray-cast image volume
(invesalius/data/volume.py), the mask preview (volume_mask.py) and the three textured slice planes
(viewer_volume.SlicePlane, Slice.UpdateSlice3D) -- and both of its volume mappers ask for
``IntermixIntersectingGeometryOn()`` (volume.py:644, volume_mask.py:52).  Here one ray per pixel carries the field's
front-to-back composite and blends every surface and slice-plane fragment at its depth: a surface hides the volume behind
it, the volume veils a surface, a slice cuts through both.

The camera is `volume.camera_for_view`'s dict, the surfaces are a `surface_view.Scene` (whose key buffers are kept: a change
of colour, transparency, preset, window / level or plane slice runs no raster stage and uploads no image, mask or mesh byte),
the field is the `DeviceVolume`'s prepared image under a composite preset, or its mask in the composite preview mode, or
nothing.

PARITY UNPINNED vs VTK's renderer (not installed): the rules S1 - S3 of DESIGN 7r are the contract; they are pinned against the
numpy restatement tests/_scene3d_ref.py.  VTK stops rays at the depth buffer of opaque geometry and draws translucent
polygons without depth order (restated from memory, unverified); here every fragment is blended where it lies.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from . import surface_view as SV
from . import volume as V

FIELD_NONE, FIELD_IMAGE, FIELD_MASK = 0, 1, 2
ORIENTATIONS = {"AXIAL": 0, "CORONAL": 1, "SAGITAL": 2}
MAX_PLANES = 3
c64 = ctypes.c_int64


class ScenePlane(ctypes.Structure):
    """struct ivx_scene_plane (include/ivx.h)."""
    _fields_ = [("picture", ctypes.c_void_p), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("orientation", ctypes.c_int32),
                ("slice", ctypes.c_int32), ("opacity", ctypes.c_float), ("reserved", ctypes.c_int32)]


def plane_shape(orientation: str, shape) -> tuple:
    """(rows, columns) of a slice picture as `slice_.get_image_slice` lays it out: AXIAL y x x, CORONAL z x x, SAGITAL z x y"""
    dz, dy, dx = (int(s) for s in shape)
    return {"AXIAL": (dy, dx), "CORONAL": (dz, dx), "SAGITAL": (dz, dy)}[orientation]


class SlicePlane:
    """One of the three slice planes of the 3-D view (viewer_volume.SlicePlane): `orientation` AXIAL / CORONAL / SAGITAL at
    slice `n`, shown with `opacity`.  `picture`: an (h, w, 3) uint8 array; None takes `DeviceVolume.show_slice(orientation,
    n, state, mask=False, download=False)` under the `DisplayState` given to `Scene3D.render` (Slice.UpdateSlice3D hands the
    2-D viewer's picture to the plane)."""

    def __init__(self, orientation: str, n: int, picture=None, opacity: float = 1.0):
        orientation = str(orientation).upper()
        if orientation not in ORIENTATIONS:
            raise ValueError("orientation must be AXIAL, CORONAL or SAGITAL")
        if not 0.0 <= float(opacity) <= 1.0:
            raise ValueError("slice plane opacity %r must lie in 0..1" % (opacity,))
        self.orientation, self.n, self.opacity = orientation, int(n), float(opacity)
        self.picture = picture

    @property
    def picture(self):
        return self._picture

    @picture.setter
    def picture(self, p):
        if p is not None:
            p = np.ascontiguousarray(p)
            if p.dtype != np.uint8 or p.ndim != 3 or p.shape[2] != 3 or p.shape[0] < 1 or p.shape[1] < 1:
                raise TypeError("a slice plane's picture is an (h, w, 3) uint8 array")
        self._picture = p
        self._uploaded = False  # (the scene's device copy is older than the picture)


def _check_planes(planes):
    planes = list(planes)
    if len(planes) > MAX_PLANES:
        raise ValueError("3-D scene: %d slice planes (at most %d)" % (len(planes), MAX_PLANES))
    names = [p.orientation for p in planes]
    if len(set(names)) != len(names):
        raise ValueError("3-D scene: two slice planes of one orientation")
    return planes


def _no_field_setup(cam: dict, background) -> dict:
    """the numbers of `volume.render_setup` a scene without a field still needs: the rays and the background"""
    origin, du, dv = V.pixel_rays(cam)
    return {"mip": False, "shade": False, "ambient": 0.0, "diffuse": 0.0, "specular": 0.0, "specular_power": 1.0,
            "alpha": np.zeros(2), "background": tuple(float(c) for c in background), "origin": origin, "du": du, "dv": dv,
            "dir": cam["dir"], "viewport": cam["viewport"], "dt": V.SAMPLE_DISTANCE, "clip": None}


def field_setup(cam: dict, spacing, scale=None, preset=None, mask_colour=None, mask_mode="composite", clip_plane=None, shade=None,
                color_lists=None, presets_dir=None, background=None, sample_distance=None):
    """(field kind, setup) of a scene: `preset` (the image's (min, max) in `scale`) -> `volume.render_setup`, `mask_colour` ->
    `volume_mask.render_setup` in the composite mode, neither -> the rays alone.  A MIP preset and the iso mode are
    ValueError: the scene composites."""
    if preset is not None and mask_colour is not None:
        raise ValueError("3-D scene: the image volume and the mask preview do not share a scene: give preset or mask_colour")
    if preset is not None:
        dt = V.SAMPLE_DISTANCE if sample_distance is None else float(sample_distance)
        if not dt > 0.0:
            raise ValueError("sample distance %r must be positive" % (sample_distance,))
        setup = V.render_setup(preset, scale, cam, clip_plane, shade, color_lists, presets_dir, dt)
        if setup["mip"]:
            raise ValueError("3-D scene: a maximum-intensity preset has no depth to blend geometry at (composite presets only)")
        if background is not None:
            setup["background"] = tuple(float(c) for c in background)
        return FIELD_IMAGE, setup
    if mask_colour is not None:
        from . import volume_mask as VM
        if mask_mode != "composite":
            raise ValueError("3-D scene: the mask preview takes part in its composite mode only (not %r)" % (mask_mode,))
        if clip_plane is not None:
            raise ValueError("3-D scene: the mask preview has no clip plane")
        return FIELD_MASK, VM.render_setup(mask_colour, "composite", cam, spacing, (0.0, 0.0, 0.0) if background is None else background,
                                           sample_distance)
    if clip_plane is not None:
        raise ValueError("3-D scene: a clip plane cuts the field, and there is none")
    return FIELD_NONE, _no_field_setup(cam, (0.0, 0.0, 0.0) if background is None else background)


def _c_planes(entries):
    """[(SlicePlane, picture pointer, h, w)] as the C table"""
    arr = (ScenePlane * MAX_PLANES)()
    for m, (pl, pointer, h, w) in zip(arr, entries):
        m.picture = pointer
        m.h, m.w, m.orientation, m.slice, m.opacity = int(h), int(w), ORIENTATIONS[pl.orientation], pl.n, pl.opacity
    return arr


class Scene3D:
    """The 3-D view's objects: `volume` (a `DeviceVolume`: its image and mask are the fields, and it makes the planes' default
    pictures), `surfaces` (a `surface_view.Scene`, or `SurfaceActor`s that become one) and `planes` (`SlicePlane`s, one per
    orientation).  The volume's prepared field and cells, the surfaces' meshes and key buffers and the planes' pictures stay
    on the device between renders.  `spacing`: the image's (sx, sy, sz) that places the planes when there is no volume."""

    def __init__(self, volume=None, surfaces=None, planes=(), spacing=None):
        self.volume = volume
        self.spacing = tuple(float(x) for x in (volume.spacing if volume is not None else (spacing or (1.0, 1.0, 1.0))))
        self._own_surfaces = surfaces is not None and not isinstance(surfaces, SV.Scene)
        stream = volume.stream if volume is not None else None
        self.surfaces = SV.Scene(surfaces, stream) if self._own_surfaces else surfaces
        self.planes = list(planes)
        self.stream = stream if stream is not None else (self.surfaces.stream if self.surfaces is not None else None)
        self._bufs = {}
        self._plane_of = {}  # buffer name -> the SlicePlane whose host picture it holds
        self._table_key = None
        self.last_render_stats = None

    def _buffer(self, name, nbytes):
        from .device import DeviceBuffer
        have = self._bufs.get(name)
        if have is None or have.nbytes < nbytes:
            if have is not None:
                have.close()
            have = self._bufs[name] = DeviceBuffer(nbytes)
        return have

    def _sync(self):
        L.check(L.lib().ivx_stream_synchronize(self.stream) if self.stream else L.lib().ivx_device_synchronize())

    def _plane_entries(self, planes, state):
        """every plane's picture on the device: a host picture is uploaded when it is new, a default one is made by
        show_slice (one launch that reads the resident image in place) and copied into the scene's own block"""
        out = []
        for pl in planes:
            name = "plane_" + pl.orientation
            if pl.picture is not None:
                h, w = pl.picture.shape[:2]
                buf = self._buffer(name, h * w * 3)
                if not pl._uploaded or self._plane_of.get(name) is not pl:
                    self._sync()  # (an earlier render may still read the block)
                    buf.upload(pl.picture)
                    pl._uploaded, self._plane_of[name] = True, pl
            else:
                if self.volume is None:
                    raise ValueError("3-D scene: a slice plane without a picture needs the volume")
                if state is None:
                    from . import slice_display as D
                    state = D.DisplayState()
                h, w = plane_shape(pl.orientation, self.volume.shape)
                shown = self.volume.show_slice(pl.orientation, pl.n, state, mask=False, download=False)
                buf = self._buffer(name, h * w * 3)
                L.check(L.lib().ivx_memcpy_d2d(buf.ptr, shown.ptr, ctypes.c_size_t(h * w * 3), self.stream), "scene plane")
                self._plane_of[name] = None
            out.append((pl, buf.ptr, h, w))
        return out

    def render(self, camera="iso", size=(512, 512), preset=None, mask_colour=None, clip_plane=None,
               interpolation=SV.SURFACE_INTERPOLATION, rgba8=False, download=True, shade=None, color_lists=None, presets_dir=None,
               background=None, state=None, mask_mode="composite", apron_value: int = 1, sample_distance=None, skip=None):
        """One picture of the scene.  `camera`: a standard view name (of the volume's image; without a volume of the
        surfaces' bounds) or a camera dict; `size` (width, height).  The field: `preset` (a composite raycasting preset, as for
        `DeviceVolume.render_volume`, with `clip_plane`, `shade`, `color_lists`, `presets_dir`) or `mask_colour` (the mask
        preview's composite mode, with `apron_value` and `sample_distance`), or neither.  `background`: r, g, b (default: the
        preset's, else black).  `state`: the `DisplayState` of the planes' default pictures.  Returns (height, width, 4)
        float32 RGBA (uint8 with `rgba8`), or the device buffer with ``download=False``; a downloading render leaves the
        sample counts in ``last_render_stats``."""
        vol = self.volume
        planes = _check_planes(self.planes)
        mode = SV._interpolation(interpolation)
        if (preset is not None or mask_colour is not None) and vol is None:
            raise ValueError("3-D scene: a field needs the volume")
        if self.surfaces is not None and len([a for a in self.surfaces.actors if a.visible]) > SV.MAX_SURFACES:
            raise ValueError("3-D scene: %d visible surfaces (at most %d)" % (len([a for a in self.surfaces.actors if a.visible]),
                                                                              SV.MAX_SURFACES))
        if vol is not None:
            vol._materialize_mask()
            cam = V.resolve_camera(camera, vol.shape, vol.spacing, size)
        else:
            if self.surfaces is None and isinstance(camera, str):
                raise ValueError("3-D scene: a view name needs a volume or surfaces to look at")
            cam = self.surfaces.camera(camera, size) if self.surfaces is not None else dict(camera, viewport=(int(size[0]), int(size[1])))
        spacing = self.spacing
        cam = dict(cam, **{k: np.asarray(cam[k], np.float64) for k in ("focal", "right", "up", "dir")})
        scale = vol._image_scale() if preset is not None else None
        kind, setup = field_setup(cam, spacing, scale, preset, mask_colour, mask_mode, clip_plane, shade, color_lists, presets_dir,
                                  background, sample_distance)
        lib = L.lib()
        field = cells = table = prefix = shape = strides = None
        apron = 0
        if kind == FIELD_IMAGE:
            vr = vol._volren_field(setup["shift"], setup["kernels"])
            rgba, _, pre = V.device_tables(setup)
            field, cells, shape = vr["vol"].ptr, vr["cells"].ptr, L.i64(vol.shape)
        elif kind == FIELD_MASK:
            from . import volume_mask as VM
            rgba, pre = VM.device_tables(setup)
            cells = vol._maskren_cells(apron_value).ptr
            field, shape, strides, apron = vol.mask.raw, L.i64(vol.shape), L.i64([vol.dy * vol.dx, vol.dx, 1]), 1
        if kind != FIELD_NONE:
            blob = np.concatenate([rgba.view(np.uint8).ravel(), pre.view(np.uint8).ravel()])
            tb = self._buffer("table", blob.nbytes)
            key = blob.tobytes()
            if self._table_key != key:  # (a camera move keeps the table: no stall)
                self._sync()  # the table buffer may still be read by the previous render
                tb.upload(blob)
                self._table_key = key
            table, prefix = tb.ptr, tb.at(rgba.nbytes)
        p = V.volren_params(setup, spacing, rgba8, skip)
        entries = self._plane_entries(planes, state)
        cplanes = _c_planes(entries)
        if self.surfaces is not None:
            runs = self.surfaces.raster_runs
            cc, visible, layers = self.surfaces.raster(cam)
            if self.surfaces.raster_runs != runs and self.surfaces.stream != self.stream:
                self.surfaces._sync()  # (the keys were made on another stream)
        else:
            cc, visible, layers = SV._c_camera(cam), [], (SV.SurfaceLayer * SV.MAX_SURFACES)()
        w, h = cam["viewport"]
        out = self._buffer("rgba8" if rgba8 else "rgba", w * h * (4 if rgba8 else 16))
        stats = self._buffer("stats", 32)
        stats.zero(self.stream, 32)
        L.check(lib.ivx_dev_scene_render(kind, field, cells, shape, strides, apron, int(apron_value), table, prefix, layers, len(visible),
                                         ctypes.byref(cc), mode, cplanes, len(entries), ctypes.byref(p), out.ptr, stats.ptr, self.stream),
                "scene_render")
        self.last_setup = setup
        if not download:
            return out
        self._sync()
        st = stats.download((4,), np.uint64)
        self.last_render_stats = {"samples": int(st[0]), "skipped": int(st[1]), "early": int(st[2]), "rays_hit": int(st[3]),
                                  "rays": w * h}
        return out.download((h, w, 4), np.uint8 if rgba8 else np.float32)

    def close(self):
        if self._own_surfaces and self.surfaces is not None:
            self.surfaces.close()
        for b in self._bufs.values():
            b.close()
        self._bufs, self._plane_of, self._table_key = {}, {}, None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def render_scene(image=None, spacing=(1.0, 1.0, 1.0), actors=(), planes=(), camera="iso", size=(512, 512), preset=None, mask=None,
                 mask_colour=None, clip_plane=None, interpolation=SV.SURFACE_INTERPOLATION, rgba8=False, shade=None, color_lists=None,
                 presets_dir=None, background=None, sample_distance=None, shape=None) -> np.ndarray:
    """Host form (ivx_scene_render): everything over PCIe and the picture back.  The field is the int16 (z, y, x) `image` under
    the composite `preset`, or the padded uint8 `mask` matrix (flag planes at index 0) in `mask_colour`, or nothing; `actors`
    are `SurfaceActor`s of host arrays, `planes` are `SlicePlane`s with pictures.  `camera`: a standard view of the image
    (`shape`: its (z, y, x) shape where neither image nor mask is given), or a camera dict."""
    planes = _check_planes(planes)
    visible = [a for a in actors if a.visible]
    if len(visible) > SV.MAX_SURFACES:
        raise ValueError("3-D scene: %d visible surfaces (at most %d)" % (len(visible), SV.MAX_SURFACES))
    if any(a.mesh is not None for a in visible):
        raise TypeError("render_scene takes host meshes: put resident ones into a Scene3D")
    mode = SV._interpolation(interpolation)
    if preset is not None:
        if image is None or image.dtype != np.int16 or image.ndim != 3:
            raise TypeError("image must be a 3-D int16 array")
        shape = image.shape
    elif mask_colour is not None:
        if mask is None or mask.dtype != np.uint8 or mask.ndim != 3 or min(mask.shape) < 2:
            raise TypeError("mask must be a 3-D uint8 matrix with its flag planes (every axis >= 2)")
        shape = tuple(int(s) - 1 for s in mask.shape)
    if isinstance(camera, str):
        if shape is not None:
            cam = V.camera_for_view(camera, shape, spacing, (int(size[0]), int(size[1])))
        else:
            from . import polydata_utils as pu
            cam = SV.camera_for_bounds(camera, SV._merge_bounds(pu.bounds(a.verts) for a in visible if len(a.verts)), size)
    else:
        cam = dict(camera, viewport=(int(size[0]), int(size[1])))
    cam = dict(cam, **{k: np.asarray(cam[k], np.float64) for k in ("focal", "right", "up", "dir")})
    scale = (int(image.min()), int(image.max())) if preset is not None else None
    kind, setup = field_setup(cam, spacing, scale, preset, mask_colour, "composite", clip_plane, shade, color_lists, presets_dir, background,
                              sample_distance)
    field = fshape = fstrides = table = prefix = None
    keep = []
    if kind == FIELD_IMAGE:
        rgba, _, pre = V.device_tables(setup)
        field, fshape, fstrides = L.ptr(image), L.i64(image.shape), L.i64(image.strides)
    elif kind == FIELD_MASK:
        from . import volume_mask as VM
        rgba, pre = VM.device_tables(setup)
        field, fshape, fstrides = L.ptr(mask), L.i64(mask.shape), L.i64(mask.strides)
    if kind != FIELD_NONE:
        table, prefix = L.ptr(rgba), L.ptr(pre)
        keep += [rgba, pre]
    for pl in planes:
        if pl.picture is None:
            raise ValueError("render_scene: a slice plane needs its picture (the default comes from a DeviceVolume)")
    cplanes = _c_planes([(pl, pl.picture.ctypes.data, pl.picture.shape[0], pl.picture.shape[1]) for pl in planes])
    layers = (SV.SurfaceLayer * SV.MAX_SURFACES)()
    for m, a in zip(layers, visible):
        m.verts, m.nverts, m.faces, m.ntris = a.verts.ctypes.data, len(a.verts), a.faces.ctypes.data, len(a.faces)
        m.normals = a.normals.ctypes.data if a.normals is not None else None
        m.rgb[:] = a.colour
        m.opacity = 1.0 - a.transparency
    p = V.volren_params(setup, spacing, rgba8)
    cc = SV._c_camera(cam)
    w, h = cam["viewport"]
    out = np.empty((h, w, 4), np.uint8 if rgba8 else np.float32)
    L.check(L.lib().ivx_scene_render(kind, field, fshape, fstrides, int(setup.get("shift", 0)), len(setup.get("kernels", ())), table, prefix,
                                     layers, len(visible), ctypes.byref(cc), mode, cplanes, len(planes), ctypes.byref(p), L.ptr(out)),
            "render_scene")
    return out
