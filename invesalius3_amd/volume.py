"""Volume rendering: the raycasting presets of the reference turned into transfer functions and a baked table.

Restates invesalius/data/volume.py (``Volume``: Create16bColorTable / Create8bColorTable / CreateOpacityTable /
Create8bOpacityTable, SetWWWL / CalculateWWWL, SetShading, SetTypeRaycasting, CalculateHistogram, TranslateScale, the
``Kernels`` and ``SHADING`` tables) and the standard views of data/viewer_volume.py (SetViewAngle, VTK's ResetCamera,
RepositionCamera) with numpy and plistlib only.  The render contract the kernels of csrc/k_volren.hip implement is in
DESIGN.md section 7d; ``render_setup`` produces everything they need from a preset, the image's range and a camera.

VTK is not installed where this was written: the node rules of vtkColorTransferFunction / vtkPiecewiseFunction (sorted by
x, a node at an existing x replaces it, piecewise linear between nodes, clamped to the end nodes), AddSegment on an empty
function, and ResetCamera's distance are restated from VTK's documentation, unverified.
"""
from __future__ import annotations

import copy
import ctypes
import math
import os
import plistlib

import numpy as np

# volume.py:52-81: vtkImageConvolve's 5x5 kernel, divided by 60.0 when set (volume.py:547)
KERNELS = {
    "Basic Smooth 5x5": (1.0, 1.0, 1.0, 1.0, 1.0,
                         1.0, 4.0, 4.0, 4.0, 1.0,
                         1.0, 4.0, 12.0, 4.0, 1.0,
                         1.0, 4.0, 4.0, 4.0, 1.0,
                         1.0, 1.0, 1.0, 1.0, 1.0),
}

# volume.py:83-107
SHADING = {
    "Default": {"ambient": 0.15, "diffuse": 0.9, "specular": 0.3, "specularPower": 15},
    "Glossy Vascular": {"ambient": 0.15, "diffuse": 0.28, "specular": 1.42, "specularPower": 50},
    "Glossy Bone": {"ambient": 0.15, "diffuse": 0.24, "specular": 1.17, "specularPower": 6.98},
    "Endoscopy": {"ambient": 0.12, "diffuse": 0.64, "specular": 0.73, "specularPower": 50},
}

# the mapper settings of LoadVolume (volume.py:675-680): SetSampleDistance(pix_diag / 5.0), SetScalarOpacityUnitDistance(pix_diag)
SAMPLE_DISTANCE = 2.0 / 5.0
OPACITY_UNIT_DISTANCE = 2.0
# early ray termination: a ray stops once its accumulated opacity reaches this
OPAQUE = 1.0 - 2.0 ** -12
CELL = 8  # macro-cell edge of the empty-space skipping grid (voxels)

# constants.py:217-278, AXIAL orientation: (view up, camera position) per standard view
VIEWS = {
    "front": ((0, 0, 1), (0, -1, 0)),
    "back": ((0, 0, 1), (0, 1, 0)),
    "right": ((0, 0, 1), (-1, 0, 0)),
    "left": ((0, 0, 1), (1, 0, 0)),
    "top": ((0, 1, 0), (0, 0, 1)),
    "bottom": ((0, -1, 0), (0, 0, -1)),
    "iso": ((0, 0, 1), (0.5, -1, 0.5)),
}


# -- presets ----------------------------------------------------------------------------------------------------------
def preset_path(name: str, presets_dir: str) -> str:
    """LoadRaycastingPreset's lookup (control.py:1422-1435) in one given directory: ``<dir>/<name>.plist``."""
    p = os.path.join(presets_dir, name + ".plist")
    if not os.path.isfile(p):
        raise FileNotFoundError("no raycasting preset %r in %s" % (name, presets_dir))
    return p


def load_preset(preset, presets_dir: str | None = None) -> dict:
    """The dict plistlib.load returns for a preset (control.py:1436-1437), from a dict (deep-copied), a ``.plist`` path,
    or a preset name looked up in `presets_dir`."""
    if isinstance(preset, dict):
        return copy.deepcopy(preset)
    preset = os.fspath(preset)
    if not preset.endswith(".plist") or not os.path.isfile(preset):
        if presets_dir is None:
            raise FileNotFoundError("raycasting preset %r: not a .plist file and no presets directory given" % preset)
        preset = preset_path(preset, presets_dir)
    with open(preset, "rb") as f:
        return plistlib.load(f, fmt=plistlib.FMT_XML)


def load_color_list(name: str, presets_dir: str) -> np.ndarray:
    """``color_list/<name>.plist`` of the presets directory as a (256, 3) float64 array of 0..255 values
    (Create8bColorTable, volume.py:406-415)."""
    path = os.path.join(presets_dir, "color_list", name + ".plist")
    if not os.path.isfile(path):
        raise FileNotFoundError("colour list %r not found in %s" % (name, os.path.join(presets_dir, "color_list")))
    with open(path, "rb") as f:
        p = plistlib.load(f, fmt=plistlib.FMT_XML)
    return np.array(list(zip(p["Red"], p["Green"], p["Blue"])), np.float64)


def _colors_8bit(preset: dict, color_lists) -> np.ndarray:
    clut = preset["CLUT"]
    if clut == "No CLUT":
        return np.repeat(np.arange(256, dtype=np.float64)[:, None], 3, 1)  # grey ramp (volume.py:417-419)
    if color_lists is None:
        raise KeyError("preset uses the colour list %r: pass color_lists (a dict or the presets directory)" % clut)
    if isinstance(color_lists, (str, os.PathLike)):
        return load_color_list(clut, os.fspath(color_lists))
    if clut not in color_lists:
        raise KeyError("unknown colour list %r" % clut)
    return np.asarray(color_lists[clut], np.float64).reshape(-1, 3)


# -- VTK transfer-function nodes --------------------------------------------------------------------------------------
class Nodes:
    """The node list of a vtkColorTransferFunction / vtkPiecewiseFunction: sorted by x, one node per x (adding a node at
    an x already present replaces its value)."""

    def __init__(self):
        self.x, self.v = [], []

    def add(self, x, *v):
        x = float(x)
        for i, xi in enumerate(self.x):
            if xi == x:
                self.v[i] = tuple(float(a) for a in v)
                return
        i = 0
        while i < len(self.x) and self.x[i] < x:
            i += 1
        self.x.insert(i, x)
        self.v.insert(i, tuple(float(a) for a in v))

    def add_segment(self, x1, y1, x2, y2):
        """vtkPiecewiseFunction::AddSegment: drops the nodes in [x1, x2], then adds both ends."""
        keep = [i for i, xi in enumerate(self.x) if not (x1 <= xi <= x2)]
        self.x = [self.x[i] for i in keep]
        self.v = [self.v[i] for i in keep]
        self.add(x1, y1)
        self.add(x2, y2)

    def array(self) -> np.ndarray:
        return np.array([(x,) + v for x, v in zip(self.x, self.v)], np.float64).reshape(len(self.x), -1)

    def evaluate(self, q) -> np.ndarray:
        """piecewise linear between nodes (midpoint 0.5, sharpness 0), clamped to the end nodes outside them"""
        a = self.array()
        q = np.asarray(q, np.float64)
        return np.stack([np.interp(q, a[:, 0], a[:, 1 + c]) for c in range(a.shape[1] - 1)], -1)


def translate_scale(scale, value):
    """TranslateScale (volume.py:737-742)"""
    return value - scale[0]


def color_nodes(preset: dict, scale, color_lists=None) -> Nodes:
    """Create16bColorTable (volume.py:379-397) or Create8bColorTable (:399-428)"""
    n = Nodes()
    if preset["advancedCLUT"]:
        for i, curve in enumerate(preset["16bitClutCurves"]):
            for j, p in enumerate(curve):
                c = preset["16bitClutColors"][i][j]
                n.add(translate_scale(scale, p["x"]), c["red"], c["green"], c["blue"])
    else:
        colors = _colors_8bit(preset, color_lists)
        ww = preset["ww"]
        wl = translate_scale(scale, preset["wl"])
        init = wl - ww / 2.0
        inc = ww / (len(colors) - 1.0)
        for k, rgb in enumerate(colors):
            n.add(init + k * inc, *[float(c) / 255.0 for c in rgb])
    return n


def opacity_nodes(preset: dict, scale) -> Nodes:
    """CreateOpacityTable (volume.py:430-463) or Create8bOpacityTable (:465-491)"""
    n = Nodes()
    n.add_segment(0, 0, 2 ** 16 - 1, 0)
    if preset["advancedCLUT"]:
        for curve in preset["16bitClutCurves"]:
            for p in curve:
                n.add(translate_scale(scale, p["x"]), p["y"])
    else:
        ww = preset["ww"]
        wl = translate_scale(scale, preset["wl"])
        n.add(wl - ww / 2.0, 0)
        n.add(wl + ww / 2.0, 1)
    return n


def set_wwwl(preset: dict, ww, wl, curve: int = 0) -> dict:
    """SetWWWL (volume.py:331-361) on a copy of `preset`; returns the new preset.  As in the reference, a curve index past
    the end falls back to curve 0."""
    p = copy.deepcopy(preset)
    if p["advancedCLUT"]:
        curves = p["16bitClutCurves"]
        try:
            c = curves[curve]
        except IndexError:
            c = curves[0]
        p1, p2 = c[0], c[-1]
        half = (p2["x"] - p1["x"]) / 2.0
        middle = p1["x"] + half
        shift_wl = wl - middle
        shift_ww = p1["x"] + shift_wl - (wl - 0.5 * ww)
        for n, i in enumerate(c):
            factor = max(abs(i["x"] - middle) / half, 0)
            i["x"] += shift_wl
            if n < len(c) / 2.0:
                i["x"] -= shift_ww * factor
            else:
                i["x"] += shift_ww * factor
    else:
        p["wl"] = wl
        p["ww"] = ww
    return p


def calculate_wwwl(preset: dict, curve: int = 0):
    """CalculateWWWL (volume.py:363-374): (ww, wl) of a 16-bit curve; an index past the end steps back by one."""
    curves = preset["16bitClutCurves"]
    try:
        c = curves[curve]
    except IndexError:
        c = curves[curve - 1]
    first, last = c[0]["x"], c[-1]["x"]
    ww = last - first
    return ww, first + ww / 2.0


def shading(preset: dict, shade: bool | None = None) -> dict:
    """SetShading (volume.py:493-504).  `shade` None follows the preset's ``useShading``, which is what a preset switch
    (``__load_preset``) does.  The first load of any preset shades regardless: LoadVolume calls ShadeOn() after
    SetShading (volume.py:691), so pass ``shade=True`` to get what the viewer shows right after loading a volume."""
    s = SHADING[preset["shading"]]
    on = bool(preset["useShading"]) if shade is None else bool(shade)
    return {"shade": on, "ambient": float(s["ambient"]), "diffuse": float(s["diffuse"]), "specular": float(s["specular"]),
            "specular_power": float(s["specularPower"])}


def is_mip(preset: dict) -> bool:
    """SetTypeRaycasting (volume.py:506-523): maximum intensity blend when the preset has ``MIP``"""
    return bool(preset.get("MIP", False))


def background(preset: dict):
    """GetBackgroundColour (volume.py:493-499): already 0..1 in the shipped presets"""
    return (float(preset["backgroundColorRedComponent"]), float(preset["backgroundColorGreenComponent"]),
            float(preset["backgroundColorBlueComponent"]))


def convolution_kernels(preset: dict) -> list:
    """ApplyConvolution (volume.py:538-563): the preset's filters in order, as 25 float64 weights k / 60.0 each"""
    out = []
    for name in preset.get("convolutionFilters", []):
        if name not in KERNELS:
            raise ValueError("unknown convolution filter %r" % name)
        out.append(np.array([k / 60.0 for k in KERNELS[name]], np.float64))
    return out


def shift_for(scale) -> int:
    """vtkImageShiftScale.SetShift(abs(scale[0])) (volume.py:626-629): the shift that makes the uint16 scalars"""
    return int(abs(scale[0]))


# -- baked table ------------------------------------------------------------------------------------------------------
def bake_table(cnodes: Nodes, onodes: Nodes, s_max: int, dt: float = SAMPLE_DISTANCE, unit: float = OPACITY_UNIT_DISTANCE):
    """One entry per integer scalar 0..s_max + 1 (the extra entry lets a sample at s_max interpolate), in float64:
    ``rgba`` (n, 4) with alpha corrected for the sample distance, a' = 1 - (1 - a)^(dt / unit); ``alpha`` (n,) the
    uncorrected a (MIP); ``prefix`` (n + 1,) uint32 with prefix[i] = number of entries below i whose a' > 0."""
    if s_max < 0 or s_max > 65535:
        raise ValueError("scalar range 0..%d outside uint16" % s_max)
    q = np.arange(s_max + 2, dtype=np.float64)
    rgb = np.clip(cnodes.evaluate(q), 0.0, 1.0)
    a = np.clip(onodes.evaluate(q)[:, 0], 0.0, 1.0)
    ac = 1.0 - np.power(1.0 - a, dt / unit)
    prefix = np.zeros(len(q) + 1, np.uint32)
    prefix[1:] = np.cumsum(ac > 0)
    return np.concatenate([rgb, ac[:, None]], 1), a, prefix


def calculate_histogram(image: np.ndarray) -> np.ndarray:
    """CalculateHistogram (volume.py:723-735): r = int(max - min) unit bins from min, so voxels equal to max fall outside
    (the accumulate's extent ends at r - 1), and r == 0 gives an empty histogram."""
    lo, hi = int(image.min()), int(image.max())
    r = int(hi - lo)
    if r <= 0:
        return np.zeros(0, np.uint64)
    v = image.ravel().astype(np.int64) - lo
    return np.bincount(v[v < r], minlength=r).astype(np.uint64)


# -- camera -----------------------------------------------------------------------------------------------------------
def volume_bounds(shape, spacing):
    """voxel (z, y, x) at world (x sx, -y sy, z sz) after to_vtk + vtkImageFlip(axis 1, about the origin): the bounds of
    the voxel centres as (xmin, xmax, ymin, ymax, zmin, zmax)"""
    dz, dy, dx = shape
    sx, sy, sz = spacing
    return (0.0, (dx - 1) * sx, -(dy - 1) * sy, 0.0, 0.0, (dz - 1) * sz)


def _norm(v):
    v = np.asarray(v, np.float64)
    n = float(np.linalg.norm(v))
    return v / n if n > 0 else v


def _reposition_scale(view, cam_pos, b, viewport):
    """RepositionCamera's fit-to-view parallel scale (viewer_volume.py:3611-3784), classified by the absolute position"""
    w_px, h_px = viewport
    xs, ys, zs = b[1] - b[0], b[3] - b[2], b[5] - b[4]
    aspect = w_px / h_px
    d = _norm(cam_pos)
    ax, ay, az = abs(d[0]), abs(d[1]), abs(d[2])
    iso = view == "iso"
    oblique = not (ay > ax and ay > az) and not (ax > ay and ax > az) and not (az > ax and az > ay)
    if iso or oblique:
        diag = math.sqrt(xs ** 2 + ys ** 2 + zs ** 2)
        width, height = math.sqrt(xs ** 2 + ys ** 2), math.sqrt(ys ** 2 + zs ** 2)
        if max(width, height) < diag * 0.8:
            if width > height:
                width = diag * 0.85
            else:
                height = diag * 0.85
    elif ay > ax and ay > az:
        width, height = xs, zs
    elif ax > ay and ax > az:
        width, height = ys, zs
    else:
        width, height = xs, ys
    if width <= 0 or height <= 0:
        return None
    obj_aspect = width / height
    scale = max((width / aspect) / 2.0, height / 2.0)
    diff = abs(obj_aspect - aspect) / max(obj_aspect, aspect)
    if iso or oblique:
        margin = 1.25 if aspect >= 1.8 else 1.28 if aspect >= 1.5 else 1.26 if aspect >= 1.3 else 1.25 if aspect >= 1.0 else 1.30
        if h_px < 400:
            margin *= 1.10
    elif diff < 0.1:
        margin = 1.15
    elif diff < 0.3:
        margin = 1.20
    else:
        margin = 1.25
    return scale * margin


def camera_for_view(view: str, shape, spacing, viewport) -> dict:
    """SetViewAngle (viewer_volume.py:3786-3865) for the AXIAL orientation: focal point 0, the view's position and view
    up, parallel projection; then VTK's ResetCamera (focal point at the bounds' centre, distance radius / sin(15 deg),
    parallel scale = radius; restated, unverified) and RepositionCamera's parallel scale.  Returns focal point, unit
    direction of projection, orthonormal screen right / up, parallel scale (half the viewport height in world units),
    camera position and the viewport."""
    return camera_from_bounds(view, volume_bounds(shape, spacing), viewport)


def camera_from_bounds(view: str, b, viewport) -> dict:
    """camera_for_view's camera of a scene with the bounds `b` = (xmin, xmax, ymin, ymax, zmin, zmax)"""
    view = view.lower()
    if view not in VIEWS:
        raise ValueError("unknown view %r (one of %s)" % (view, ", ".join(VIEWS)))
    w_px, h_px = int(viewport[0]), int(viewport[1])
    if w_px <= 0 or h_px <= 0:
        raise ValueError("viewport %r must be positive" % (viewport,))
    up, pos = VIEWS[view]
    center = np.array([(b[0] + b[1]) / 2, (b[2] + b[3]) / 2, (b[4] + b[5]) / 2])
    vpn = _norm(pos)  # focal point 0 -> position
    w = np.array([b[1] - b[0], b[3] - b[2], b[5] - b[4]])
    radius = float(np.sqrt((w * w).sum())) * 0.5
    if radius == 0.0:
        radius = 1.0
    dist = radius / math.sin(math.radians(30.0) * 0.5)
    position = center + dist * vpn
    d = -vpn
    right = _norm(np.cross(d, np.asarray(up, np.float64)))
    upv = _norm(np.cross(right, d))  # the view up made orthogonal to the direction
    scale = _reposition_scale(view, position, b, (w_px, h_px))
    return {"view": view, "focal": center, "dir": d, "right": right, "up": upv, "position": position,
            "parallel_scale": radius if scale is None else scale, "viewport": (w_px, h_px)}


def resolve_camera(view, shape, spacing, size) -> dict:
    """A standard view name as camera_for_view's camera of the image `shape`, or a camera dict as it is; either way
    with the viewport `size` (width, height)."""
    viewport = (int(size[0]), int(size[1]))
    if isinstance(view, str):
        return camera_for_view(view, shape, spacing, viewport)
    return dict(view, viewport=viewport)


def pixel_rays(cam: dict):
    """World position of pixel (0, 0)'s centre on the plane through the focal point, and the steps per column / row
    (row 0 is the top of the viewport)."""
    w_px, h_px = cam["viewport"]
    px = 2.0 * cam["parallel_scale"] / h_px
    du = cam["right"] * px
    dv = -cam["up"] * px
    origin = cam["focal"] + du * (0.5 - w_px / 2.0) + dv * (0.5 - h_px / 2.0)
    return origin, du, dv


# -- everything one render needs --------------------------------------------------------------------------------------
def render_setup(preset, scale, camera: dict, clip_plane=None, shade: bool | None = None, color_lists=None,
                 presets_dir: str | None = None, dt: float = SAMPLE_DISTANCE, unit: float = OPACITY_UNIT_DISTANCE) -> dict:
    """The preset (anything load_preset takes), the image's (min, max) and a camera (camera_for_view) as the numbers the
    kernels take.  `clip_plane`: (normal, origin) in world coordinates; what has n . (p - o) >= 0 is kept.
    `color_lists`: a dict name -> (256, 3) values, or a presets directory (default: `presets_dir`)."""
    p = load_preset(preset, presets_dir)
    lo, hi = int(scale[0]), int(scale[1])
    shift = shift_for((lo, hi))
    s_max = hi + shift
    if color_lists is None:
        color_lists = presets_dir
    rgba, alpha, prefix = bake_table(color_nodes(p, (lo, hi), color_lists), opacity_nodes(p, (lo, hi)), s_max, dt, unit)
    origin, du, dv = pixel_rays(camera)
    sh = shading(p, shade)
    mip = is_mip(p)
    out = {"preset": p, "scale": (lo, hi), "shift": shift, "kernels": convolution_kernels(p), "rgba": rgba,
           "alpha": alpha, "prefix": prefix, "mip": mip, "shade": sh["shade"] and not mip, "ambient": sh["ambient"],
           "diffuse": sh["diffuse"], "specular": sh["specular"], "specular_power": sh["specular_power"],
           "background": background(p), "origin": origin, "du": du, "dv": dv, "dir": camera["dir"],
           "viewport": camera["viewport"], "dt": float(dt), "clip": None}
    if clip_plane is not None:
        n, o = clip_plane
        out["clip"] = (np.asarray(n, np.float64).reshape(3), np.asarray(o, np.float64).reshape(3))
    return out


def to_rgba8(img: np.ndarray) -> np.ndarray:
    """float RGBA in 0..1 -> uint8, floor(255 v + 0.5) clamped"""
    return np.clip(np.floor(255.0 * np.asarray(img, np.float64) + 0.5), 0, 255).astype(np.uint8)


def write_png(path: str, rgba8: np.ndarray):
    """An 8-bit RGBA PNG with zlib and struct only"""
    import struct
    import zlib

    h, w = rgba8.shape[:2]
    raw = b"".join(b"\x00" + rgba8[r].tobytes() for r in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def read_png(path: str) -> np.ndarray:
    """The inverse of write_png (8-bit RGBA, filter type 0 rows only)"""
    import struct
    import zlib

    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", None, None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w)
    if np.any(raw[:, 0] != 0):
        raise ValueError("read_png reads unfiltered rows only")
    return raw[:, 1:].reshape(h, w, 4).copy()


# -- the C ABI --------------------------------------------------------------------------------------------------------
def skip_enabled() -> bool:
    """IVX_VR_SKIP=0 turns empty-space skipping off (a diagnostic switch: it changes no bit of the result)"""
    return os.environ.get("IVX_VR_SKIP", "1") != "0"


def volren_params(setup: dict, spacing, out_u8: bool = False, skip: bool | None = None):
    """struct ivx_volren_params for `setup` (render_setup)"""
    from . import _lib as L

    p = L.VolrenParams()
    p.width, p.height = setup["viewport"]
    p.mip, p.shade = int(setup["mip"]), int(setup["shade"])
    p.skip = int(skip_enabled() if skip is None else skip)
    p.n_table = len(setup["alpha"])
    p.out_u8 = int(out_u8)
    for name in ("origin", "du", "dv", "dir"):
        getattr(p, name)[:] = [float(v) for v in setup[name]]
    p.spacing[:] = [float(v) for v in spacing]
    p.dt = setup["dt"]
    p.ambient, p.diffuse, p.specular, p.specular_power = (setup["ambient"], setup["diffuse"], setup["specular"],
                                                          setup["specular_power"])
    p.background[:] = list(setup["background"])
    if setup["clip"] is not None:
        p.clip = 1
        p.clip_normal[:] = [float(v) for v in setup["clip"][0]]
        p.clip_origin[:] = [float(v) for v in setup["clip"][1]]
    return p


def device_tables(setup: dict):
    """the baked table as the kernels read it: float32 (n, 4), float32 (n,), uint32 (n + 1,)"""
    return (np.ascontiguousarray(setup["rgba"], np.float32), np.ascontiguousarray(setup["alpha"], np.float32),
            np.ascontiguousarray(setup["prefix"], np.uint32))


def volume_render(image: np.ndarray, spacing, preset, view="iso", size=(512, 512), clip_plane=None, shade=None,
                  color_lists=None, presets_dir=None, rgba8: bool = False) -> np.ndarray:
    """Host form (ivx_volume_render): the int16 (z, y, x) image over PCIe, rendered with `preset` from a standard `view`
    (or a camera dict from camera_for_view) at `size`; returns (H, W, 4) float32 RGBA, or uint8 with `rgba8`."""
    from . import _lib as L

    if image.dtype != np.int16 or image.ndim != 3:
        raise TypeError("image must be a 3-D int16 array")
    cam = resolve_camera(view, image.shape, spacing, size)
    setup = render_setup(preset, (int(image.min()), int(image.max())), cam, clip_plane, shade, color_lists, presets_dir)
    rgba, alpha, prefix = device_tables(setup)
    p = volren_params(setup, spacing, rgba8)
    w, h = setup["viewport"]
    out = np.empty((h, w, 4), np.uint8 if rgba8 else np.float32)
    L.check(L.lib().ivx_volume_render(L.ptr(image), L.i64(image.shape), L.i64(image.strides), int(setup["shift"]),
                                      len(setup["kernels"]), L.ptr(rgba), L.ptr(alpha), L.ptr(prefix), ctypes.byref(p),
                                      L.ptr(out)), "volume_render")
    return out
