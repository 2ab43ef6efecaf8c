"""Inputs of the 3-D scene's tests, shared by the CPU tests (the restatement against hand numbers and against the
host build of csrc/scene3d_math.h) and the GPU tests: two small volumes, the mask matrix, cameras, quads that face the camera,
slice pictures and the list of scenes.

A case is a dict: name, kind (R3.NONE / IMAGE / MASK), img or matrix, spacing, view, size, preset / colour, layers
(tests/_surface_view_ref.layer), planes (tests/_scene3d_ref.plane), clip, mode, dt."""
import functools

import numpy as np

import _maskren_ref as MR
import _scene3d_ref as R3
import _surface_view_cases as SC
import _surface_view_ref as SR
import _volren_ref as R

SPACING = (0.9, 0.7, 1.3)
SHAPES = {"small": (9, 10, 11), "cells": (20, 24, 28)}  # the second crosses a macro cell of 8 on every axis
SIZES = {"partial": (19, 13), "full": (64, 48)}         # partial tiles on both axes; whole tiles
BACKGROUND = (0.125, 0.25, 0.5)
PRESETS, CLUTS, _ = R.fixture()
GREEN, RED, BLUE = (0.33, 1.0, 0.33), (1.0, 0.33, 0.33), (0.25, 0.5, 1.0)


def simple_preset(ww, wl, shade=False, background=BACKGROUND):
    """an 8-bit preset: a grey ramp of width ww about wl, opacity 0 below and 1 above it"""
    return {"advancedCLUT": False, "CLUT": "No CLUT", "ww": float(ww), "wl": float(wl), "shading": "Default", "useShading": bool(shade),
            "MIP": False, "convolutionFilters": [], "backgroundColorRedComponent": background[0],
            "backgroundColorGreenComponent": background[1], "backgroundColorBlueComponent": background[2]}


def solid_preset(background=BACKGROUND):
    """a 16-bit preset whose one curve holds opacity 1 from -900 up: the first sample in material ends the ray"""
    colour = {"red": 1.0, "green": 0.8, "blue": 0.6}
    return {"advancedCLUT": True, "16bitClutCurves": [[{"x": -900.0, "y": 1.0}, {"x": 4000.0, "y": 1.0}]],
            "16bitClutColors": [[dict(colour), dict(colour)]], "shading": "Default", "useShading": False, "MIP": False,
            "convolutionFilters": [], "backgroundColorRedComponent": background[0], "backgroundColorGreenComponent": background[1],
            "backgroundColorBlueComponent": background[2]}


OPAQUE_PRESET = solid_preset()                 # everything inside the synthetic volume's empty shell is opaque at once
HAZE_PRESET = simple_preset(8000.0, 1000.0)    # a thin haze everywhere: no ray ends early


@functools.lru_cache(maxsize=None)
def image(which):
    img = R.synth_volume(SHAPES[which], seed=7)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def mask_matrix():
    """the padded 10 x 11 x 12 matrix of a thresholded 9 x 10 x 11 volume"""
    m = MR.padded(MR.thresholded(R.synth_volume(SHAPES["small"], seed=7, shell=2), 0, 3071))
    m.setflags(write=False)
    return m


def camera(view, shape, spacing, size):
    from invesalius3_amd import volume as V
    return V.camera_for_view(view, shape, spacing, size)


def cam_frame(cam):
    return [np.asarray(cam[k], np.float64) for k in ("focal", "right", "up", "dir")]


def facing_quad(cam, t, half=(4.0, 3.0), centre=(0.0, 0.0)):
    """two triangles that face the camera at depth t (world units from the focal plane): centre and half sizes along the
    screen's right / up"""
    f, r, u, d = cam_frame(cam)
    c = f + centre[0] * r + centre[1] * u + t * d
    v = np.array([c - half[0] * r - half[1] * u, c + half[0] * r - half[1] * u, c + half[0] * r + half[1] * u,
                  c - half[0] * r + half[1] * u], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    if not (SR.raster_keys(v, faces, cam) != SR.EMPTY).any():
        faces = np.ascontiguousarray(faces[:, ::-1])
    return v, faces


def sphere(shape, spacing, radius, level=2):
    """an icosphere about the volume's centre with its analytic normals"""
    from invesalius3_amd import volume as V
    b = V.volume_bounds(shape, spacing)
    return SC.icosphere(radius, level, ((b[0] + b[1]) / 2, (b[2] + b[3]) / 2, (b[4] + b[5]) / 2))


def slice_picture(orientation, shape, seed=3):
    """a picture of the slice's layout with every byte different from its neighbours"""
    dz, dy, dx = shape
    h, w = {"AXIAL": (dy, dx), "CORONAL": (dz, dx), "SAGITAL": (dz, dy)}[orientation]
    return np.random.default_rng(seed + len(orientation)).integers(0, 256, (h, w, 3), dtype=np.uint8)


def three_planes(shape, opacity=1.0, at=None):
    at = at or {"AXIAL": shape[0] // 2, "CORONAL": shape[1] // 2, "SAGITAL": shape[2] // 2}
    return [R3.plane(o, at[o], slice_picture(o, shape), opacity) for o in ("AXIAL", "CORONAL", "SAGITAL")]


def _case(name, kind, which="small", view="iso", size="partial", preset=None, colour=None, layers=(), planes=(), clip=None,
          mode=SR.GOURAUD, dt=None, shade=None, spacing=SPACING):
    shape = SHAPES[which]
    return {"name": name, "kind": kind, "which": which, "shape": shape, "spacing": spacing, "view": view, "size": SIZES[size],
            "preset": preset, "colour": colour, "layers": list(layers), "planes": list(planes), "clip": clip, "mode": mode, "dt": dt,
            "shade": shade, "cam": camera(view, shape, spacing, SIZES[size])}


def cases():
    L = SR.layer
    out = []
    # the pictures: both fields, both viewports, three views, surfaces inside and planes through the field
    for which, size in (("small", "partial"), ("cells", "full")):
        shape = SHAPES[which]
        for view in ("front", "top", "iso"):
            v, f, nrm = sphere(shape, SPACING, 0.3 * min((s - 1) * sp for s, sp in zip(shape[::-1], SPACING)))
            cam = camera(view, shape, SPACING, SIZES[size])
            qv, qf = facing_quad(cam, -1.0, (3.0, 2.0), (1.0, 0.5))
            out.append(_case("%s %s scene" % (which, view), R3.IMAGE, which, view, size, PRESETS["Bone + Skin"],
                             layers=[L(v, f, nrm, colour=GREEN), L(qv, qf, colour=RED, transparency=0.5)], planes=three_planes(shape, 0.75),
                             shade=True))
    # empty macro cells in front of and around the material (the Standard preset leaves the field's corner cells empty), with a wide
    # translucent quad and the planes inside them: jumps happen and are capped at K_f
    shape = SHAPES["cells"]
    cam = camera("iso", shape, SPACING, SIZES["full"])
    out.append(_case("cells iso skipping", R3.IMAGE, "cells", "iso", "full", PRESETS["Standard"],
                     layers=[L(*facing_quad(cam, -7.0, (14.0, 11.0)), colour=RED, transparency=0.6),
                             L(*sphere(shape, SPACING, 4.0), colour=GREEN)], planes=three_planes(shape, 0.75, {"AXIAL": 3, "CORONAL": 20, "SAGITAL": 4})))
    shape = SHAPES["small"]
    cam = camera("iso", shape, SPACING, SIZES["partial"])
    # all eleven fragments on one pixel: eight stacked translucent quads and the three planes
    stack = [L(*facing_quad(cam, -3.0 + 0.7 * k, (2.5, 2.5)), colour=SC_colour(k), transparency=0.6) for k in range(8)]
    out.append(_case("eleven fragments", R3.IMAGE, preset=HAZE_PRESET, layers=stack, planes=three_planes(shape, 0.5)))
    front = camera("front", shape, SPACING, SIZES["partial"])
    far = 0.5 * (shape[1] - 1) * SPACING[1] + 2.0
    out.append(_case("fragment before the box", R3.IMAGE, view="front", preset=HAZE_PRESET,
                     layers=[L(*facing_quad(front, -far), colour=RED, transparency=0.5)]))
    out.append(_case("fragment behind the box", R3.IMAGE, view="front", preset=HAZE_PRESET,
                     layers=[L(*facing_quad(front, far), colour=RED, transparency=0.5)]))
    out.append(exact_sample_case())
    out.append(_case("surface beside the box", R3.IMAGE, view="front", preset=HAZE_PRESET,
                     layers=[L(*facing_quad(front, 0.0, (1.0, 1.0), (0.5 * (shape[2] - 1) * SPACING[0] + 2.0, 0.0)), colour=BLUE)]))
    out.append(_case("nothing anywhere", R3.NONE))
    out.append(_case("opaque surface in front", R3.IMAGE, view="front", preset=PRESETS["Bone + Skin"], shade=True,
                     layers=[L(*facing_quad(front, -far, (20.0, 20.0)), colour=GREEN)]))
    out.append(_case("opaque preset hides the surface", R3.IMAGE, size="full", preset=OPAQUE_PRESET,
                     layers=[L(*sphere(shape, SPACING, 0.6), colour=RED)]))
    from invesalius3_amd import volume as V
    b = V.volume_bounds(shape, SPACING)
    o = np.array([(b[0] + b[1]) / 2, (b[2] + b[3]) / 2, (b[4] + b[5]) / 2])
    n = -np.array([1.0, -0.4, 0.3]) / np.linalg.norm([1.0, -0.4, 0.3])  # (against the iso view: the NEAR half goes)
    out.append(_case("clip plane", R3.IMAGE, preset=PRESETS["Bone + Skin"], clip=(n, o),
                     layers=[L(*sphere(shape, SPACING, 2.5), colour=GREEN)]))
    out.append(_case("mask field", R3.MASK, colour=(0.9, 0.8, 0.2), layers=[L(*sphere(shape, SPACING, 2.0), colour=BLUE, transparency=0.3)],
                     planes=[R3.plane("AXIAL", 4, slice_picture("AXIAL", shape), 0.8)]))
    out.append(_case("surfaces and planes alone", R3.NONE, layers=[L(*sphere(shape, SPACING, 2.5), colour=GREEN, transparency=0.4)],
                     planes=three_planes(shape)))
    return out


def SC_colour(k):
    from invesalius3_amd import surface_view
    return surface_view.SURFACE_COLOUR[k]


def exact_sample_case():
    """Front view, unit spacing, dt = 0.5: the rays enter the 9 x 10 x 11 box at tin = -4.5 exactly, and a quad at world
    y = -2.5 has t = 2.0 = tin + 13 dt: the fragment goes before sample 13"""
    shape = SHAPES["small"]
    sp = (1.0, 1.0, 1.0)
    cam = camera("front", shape, sp, SIZES["partial"])
    f = cam_frame(cam)[0]
    assert f[1] == -4.5
    quad = facing_quad(cam, 2.0, (2.0, 2.0))
    assert np.all(quad[0][:, 1] == np.float32(-2.5))
    return _case("fragment on a sample", R3.IMAGE, view="front", preset=HAZE_PRESET, dt=0.5, spacing=sp,
                 layers=[SR.layer(*quad, colour=RED, transparency=0.5)])


# ---- a case as the restatement's and the product's arguments -----------------------------------------------------------------
def setup_of(case):
    """(field, setup) of the restatement for a case"""
    from invesalius3_amd import scene3d as S3
    from invesalius3_amd import volume_mask as VM
    cam = dict(case["cam"])
    if case["kind"] == R3.IMAGE:
        img = image(case["which"])
        kw = {} if case["dt"] is None else {"sample_distance": case["dt"]}
        kind, setup = S3.field_setup(cam, case["spacing"], (int(img.min()), int(img.max())), case["preset"], clip_plane=case["clip"],
                                     shade=case["shade"], color_lists=CLUTS, **kw)
        return prepared(case["which"], setup["shift"], len(setup["kernels"])), setup
    if case["kind"] == R3.MASK:
        return mask_matrix(), VM.render_setup(case["colour"], "composite", cam, case["spacing"], BACKGROUND, case["dt"])
    return None, S3.field_setup(cam, case["spacing"], background=BACKGROUND)[1]


@functools.lru_cache(maxsize=None)
def prepared(which, shift, nsmooth):
    from invesalius3_amd import volume as V
    w = V.convolution_kernels({"convolutionFilters": ["Basic Smooth 5x5"] * nsmooth})
    out = R.prepare(image(which), shift, w)
    out.setflags(write=False)
    return out


def capped_jumps(case):
    """how many fragments lie strictly inside a jump: samples K_f - 1 and K_f both exist and sit in one macro cell that the
    preset leaves empty, so an uncapped jump from K_f - 1 would pass the fragment"""
    field, setup = setup_of(case)
    ref = reference(case)
    A, B, hi, tin, kmax = R.rays(field.shape, case["spacing"], setup)
    cells = R.cells(field).astype(np.int64)
    nt, prefix = len(setup["alpha"]), setup["prefix"]
    count = 0
    for layer in range(R3.MAX_FRAGS):
        kf = ref["kf"][layer]
        for ray in np.nonzero((kf >= 1) & (kf <= kmax))[0]:
            pos = [np.clip(A[ray] + (tin[ray] + k * setup["dt"]) * B, 0.0, hi) for k in (kf[ray] - 1, kf[ray])]
            ca, cb = [tuple(int(v) // R.CELL for v in p[::-1]) for p in pos]  # (cz, cy, cx)
            mn, mx = cells[ca]
            count += int(ca == cb and prefix[min(mx + 1, nt - 1) + 1] == prefix[max(mn - 1, 0)])
    return count


_REF = {}


def reference(case):
    """the restatement's result of a case: computed once, shared, never modified"""
    if case["name"] not in _REF:
        field, setup = setup_of(case)
        ref = R3.render(field, case["spacing"], setup, case["layers"], case["cam"], case["mode"], case["planes"], case["kind"])
        for v in ref.values():
            v.setflags(write=False)
        _REF[case["name"]] = ref
    return _REF[case["name"]]
