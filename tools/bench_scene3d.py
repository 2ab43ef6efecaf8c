"""Device times of the 3-D scene (k_scene3d.hip) on the bench volume: synth_v512, "Bone + Skin" and "Gold Bone" shaded, the
largest part of the bench surface (threshold 226 .. 3071) with its point normals, 1024^2 and 2048^2, Front and Iso.  In one
process, HIP events, 2 warm-ups, medians of five, microseconds:
  (a) the parent's three separate calls: render_volume, Scene.render (raster + resolve), show_slice x 3
  (b) the scene with the field alone                       (expectation: within 1 - 2 % of render_volume)
  (c) the scene with the opaque surface                     (expectation: below the sum in (a): rays end at the surface)
  (d) the scene with the surface at transparency 0.5 and the three planes
Presets come from tests/golden/ref_volume.npz.
python tools/bench_scene3d.py [n] [--out profiles/bench_scene3d_512.json]"""
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import _volren_ref as R  # noqa: E402
from bench import synth_v512  # noqa: E402
from invesalius3_amd import _lib as L  # noqa: E402
from invesalius3_amd import polydata_utils as pu  # noqa: E402
from invesalius3_amd import scene3d as S3  # noqa: E402
from invesalius3_amd import slice_display as D  # noqa: E402
from invesalius3_amd import surface_process as sp  # noqa: E402
from invesalius3_amd import surface_view as SV  # noqa: E402
from invesalius3_amd.device import DeviceVolume  # noqa: E402

WARM, REPS = 2, 5
SPACING = (0.5, 0.5, 0.5)
THRESHOLD = (226, 3071)


def timed(vol, name, fn):
    """median device time of fn in us"""
    for k in range(WARM + REPS):
        if k == WARM:
            vol.sync()
            vol.timer.collect()  # drops the warm-up spans
        if k < WARM:
            fn()
        else:
            with vol.timer.span(name):
                fn()
    vol.sync()
    return round(statistics.median(vol.timer.collect()[name]) * 1e3, 2)  # ms -> us


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 512
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/bench_scene3d_%d.json" % n
    presets, cluts, _ = R.fixture()
    img = np.ascontiguousarray(synth_v512((n, n, n)))
    res = {"volume": [n, n, n], "spacing": list(SPACING), "threshold": list(THRESHOLD), "device": L.device_name(), "warmup": WARM,
           "reps": REPS, "unit": "us", "runs": []}
    state = D.DisplayState(window_width=2000.0, window_level=300.0)
    slices = (("AXIAL", n // 2), ("CORONAL", n // 2), ("SAGITAL", n // 2))
    with DeviceVolume(img, spacing=SPACING) as vol:
        vol.threshold(*THRESHOLD)
        whole = pu.DeviceMesh.from_volume(vol, vol.marching_cubes_indexed(from_binary=True, fill_border_holes=True))
        part = whole.keep_largest()
        vol.sync()
        verts, faces = part.download()
        part.close()
        verts, faces, normals, _ = sp.point_normals(verts, faces)
        res["vertices"], res["triangles"] = len(verts), len(faces)
        actor = SV.SurfaceActor(verts, faces, normals)
        with SV.Scene([actor], vol.stream) as surfaces, S3.Scene3D(vol) as alone, S3.Scene3D(vol, surfaces) as with_surface, \
                S3.Scene3D(vol, surfaces, [S3.SlicePlane(o, k) for o, k in slices]) as everything:
            for preset in ("Bone + Skin", "Gold Bone"):
                for view in ("front", "iso"):
                    for size in (1024, 2048):
                        kw = dict(preset=presets[preset], color_lists=cluts, shade=True, download=False)
                        rec = {"preset": preset, "view": view, "size": size}
                        actor.transparency = 0.0
                        rec["a_render_volume"] = timed(vol, "a1", lambda: vol.render_volume(presets[preset], view, (size, size), shade=True,
                                                                                             color_lists=cluts, download=False))
                        rec["a_surface_resolve"] = timed(vol, "a2", lambda: surfaces.render(view, (size, size), vol.shape, SPACING, download=False))
                        surfaces.invalidate()
                        rec["a_surface_raster_and_resolve"] = timed(vol, "a2r", lambda: (surfaces.invalidate(), surfaces.render(
                            view, (size, size), vol.shape, SPACING, download=False)))
                        rec["a_show_slice_x3"] = timed(vol, "a3", lambda: [vol.show_slice(o, k, state, mask=False, download=False) for o, k in slices])
                        rec["a_sum"] = round(rec["a_render_volume"] + rec["a_surface_resolve"] + rec["a_show_slice_x3"], 2)
                        rec["b_scene_field_alone"] = timed(vol, "b", lambda: alone.render(view, (size, size), **kw))
                        rec["c_scene_opaque_surface"] = timed(vol, "c", lambda: with_surface.render(view, (size, size), **kw))
                        actor.transparency = 0.5
                        rec["d_scene_translucent_and_planes"] = timed(vol, "d", lambda: everything.render(view, (size, size), state=state, **kw))
                        rec["b_over_render_volume"] = round(rec["b_scene_field_alone"] / rec["a_render_volume"], 4)
                        rec["c_over_a_sum"] = round(rec["c_scene_opaque_surface"] / rec["a_sum"], 4)
                        res["runs"].append(rec)
                        print(json.dumps(rec), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
