"""Headless driver: a .inv3 project in, mask / surface / measurements out, every voxel and triangle stage on the GPU.

    python -m invesalius3_amd.headless CASE.inv3 --threshold 226 3071 --seed 250 260 100 --largest --smooth \\
        --stl bone.stl --save CASE_out.inv3
    python -m invesalius3_amd.headless CASE.inv3 --threshold 226 3071 --largest --remove-nonvisible --stl shell.stl
    python -m invesalius3_amd.headless CASE.inv3 --threshold 226 3071 --surface-seed 120.5 98.0 40.0 --stl part.stl
    python -m invesalius3_amd.headless CASE.inv3 --threshold 226 3071 --split parts/ --split-min-triangles 100
    python -m invesalius3_amd.headless CASE.inv3 --threshold 226 3071 --largest --geodesic 120.5 98 40 80 60.5 75 --geodesic-npy path.npy
    python -m invesalius3_amd.headless CASE.inv3 --filter median 3 --threshold 226 3071 --stl bone.stl
    python -m invesalius3_amd.headless CASE.inv3 --segment brain --weights brain_mri_t1.pt --stl brain.stl
    python -m invesalius3_amd.headless CASE.inv3 --render "Bone + Skin" --presets-dir DIR --view iso --png out.png
    python -m invesalius3_amd.headless CASE.inv3 --threshold 226 3071 --mask-preview iso --mask-colour 0 1 0 --png mask.png
    python -m invesalius3_amd.headless CASE.inv3 --threshold 226 3071 --largest --view iso --surface-png bone.png --surface-interpolation phong
    python -m invesalius3_amd.headless CASE.inv3 --threshold 226 3071 --show-slice AXIAL 40 --window 2000 300 --colour-table Rainbow --png slice.png
    python -m invesalius3_amd.headless CASE.inv3 --density-ellipse AXIAL 40 120 98 40 140 98 40 120 110 40 --remeasure --measures-json m.json --save CASE_out.inv3
    python -m invesalius3_amd.headless --import-surface part.stl --largest --stl out.stl
    python -m invesalius3_amd.headless CASE.inv3 --import-surface scanner.ply --import-world --split parts/

What the reference does through its GUI for the same result: Slice.SetMaskThreshold / do_threshold_to_all_slices
(invesalius/data/slice_.py:1240-1247, 1739-1769), the Image Filters dialog (slice_.py:2330-2539), the deep-learning segmentation (segmentation/deep_learning/segment.py), the 3-D view's volume rendering (data/volume.py:575-707), the region-growing tool (styles.py:3151-3216),
SurfaceManager.AddNewActor -> create_surface_piece / join_process_surface (surface.py:1362-1380,
surface_process.py:71-472), Remove non-visible faces (polydata_utils.py:363-455), the surface connectivity tools (Surface.OnSplitSurface / OnSeedSurface, surface.py:319-411) and vtkSTLWriter (surface.py:1827-1829).  No wx, no VTK here; one JSON line on stdout."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

from . import _lib as L
from . import project as prj
from . import resident
from . import surface_process as sp
from .device import DeviceVolume, c64


# --filter NAME -> the reference's filter_type (slice_.py:2370-2381)
FILTER_TYPES = {"gaussian": 0, "median": 1, "mean": 2, "sharpen": 3, "despeckle": 4, "border": 5}


def run(args) -> dict:
    t_all = time.perf_counter()
    proj = prj.open_inv3(args.project)
    out = {"project": proj.name, "shape": list(proj.matrix_shape), "spacing": list(proj.spacing), "dtype": proj.matrix_dtype}
    if proj.matrix.dtype != np.int16:
        raise TypeError("the GPU path takes int16 volumes (found %s)" % proj.matrix.dtype)
    bound = [resident.bind(proj.matrix)]  # the project's image, and below the mask the run works on, for its length
    _image_geometry(args, proj, bound, out)
    vol = DeviceVolume(proj.matrix, spacing=proj.spacing)
    lib = L.lib()
    try:
        filtered = None
        if args.filter is not None:
            # the Image Filters dialog (Slice.__apply_image_filter, slice_.py:2330-2430) on the resident image
            ftype, fvalue = FILTER_TYPES[args.filter[0]], float(args.filter[1])
            dimension, orientation = ("3D", "Axial") if args.filter_2d is None else ("2D", args.filter_2d.capitalize())
            with vol.timer.span("filter"):
                vol.filter_image(ftype, fvalue, dimension, orientation)
            out["filter"] = {"type": args.filter[0], "value": fvalue, "dimension": dimension, "orientation": orientation}
            if args.save:
                vol.sync()
                filtered = (vol.image.download(vol.shape, np.int16), ftype, fvalue, dimension, orientation)
        if args.render is not None:
            # the 3-D view (Volume.LoadVolume + the viewer's SetViewAngle, volume.py:575-707) of the resident image
            from . import volume as V
            pdir = args.presets_dir
            if pdir is None and args.render.endswith(".plist"):
                pdir = os.path.dirname(os.path.abspath(args.render))  # its colour lists sit next to it
            w, h = args.size
            with vol.timer.span("render"):
                rgba8 = vol.render_volume(args.render, args.view, (w, h), presets_dir=pdir, rgba8=True)
            out["render"] = {"preset": args.render, "view": args.view, "size": [w, h], **vol.last_render_stats}
            if args.png:
                V.write_png(args.png, rgba8)
                out["render"]["png"] = args.png
            if _render_only(args):
                out["gpu_ms"] = {k: round(float(sum(v)), 4) for k, v in vol.timer.collect().items()}
                return out
        if _measures_asked(args):
            _density(args, proj, vol, out)
            if _measure_only(args):
                if args.save:
                    prj.save_inv3(args.save, proj)
                    out["saved"] = args.save
                out["gpu_ms"] = {k: round(float(sum(v)), 4) for k, v in vol.timer.collect().items()}
                return out
        if args.show_slice is not None and _show_only(args):
            _show_slice(args, proj, vol, False, out)  # no mask was asked for: the image alone
            out["gpu_ms"] = {k: round(float(sum(v)), 4) for k, v in vol.timer.collect().items()}
            return out
        segmented = False
        if args.segment is not None:
            # the Segmentation menu's deep-learning tool (BrainSegmentProcess / TracheaSegmentProcess, segment.py:505-541,
            # 919-953) into the resident mask: probabilities, then apply_segment_threshold
            from . import segment as SG
            pre = SG.PRESETS[args.segment]
            wwwl = args.apply_wwwl is not None
            ww, wl = args.apply_wwwl if wwwl else (255, 127)
            with vol.timer.span("segment"):
                vol.segment_unet3d(args.weights, overlap=args.overlap, patch_size=pre.patch_size, apply_wwwl=wwwl,
                                   window_width=ww, window_level=wl)
            with vol.timer.span("segment_threshold"):
                vol.apply_segment_threshold(args.seg_threshold)
            out["segment"] = {"tool": pre.name, "weights": str(args.weights), "overlap": args.overlap,
                              "patch_size": pre.patch_size, "threshold": args.seg_threshold,
                              "apply_wwwl": [ww, wl] if wwwl else None}
            lo, hi = 0, 0
            segmented = True
        elif args.threshold is not None:
            lo, hi = args.threshold
            with vol.timer.span("threshold"):
                vol.threshold(lo, hi)
            out["threshold"] = [lo, hi]
        else:
            if args.mask not in proj.masks:
                raise KeyError("project holds no mask %d (masks: %s)" % (args.mask, sorted(proj.masks)))
            rec = proj.masks[args.mask]
            bound.append(resident.bind(rec.matrix))
            vol.mask.upload_view(rec.interior)
            lo, hi = rec.threshold_range
            out["mask"] = {"index": args.mask, "name": rec.name, "threshold_range": [lo, hi]}
        if args.seed:
            if args.threshold is None and rec.edited:
                # the region is grown in the IMAGE inside the mask's threshold range; an edited mask (brush, cut, earlier
                # region growing) is no longer that threshold, and growing would silently throw the edits away
                raise SystemExit("--seed with --mask %d: that mask was edited by hand; region growing floods the image inside "
                                 "the mask's threshold range and would discard the edits -- use --threshold LO HI instead"
                                 % args.mask)
            seeds = [tuple(args.seed[i:i + 3]) for i in range(0, len(args.seed), 3)]
            strct = np.ones((3, 3, 3), np.uint8) if args.connectivity == 26 else _strct(args.connectivity)
            vol.zero_out_mask()
            with vol.timer.span("region_grow"):
                rounds = vol.region_grow(seeds, lo, hi, strct, fill=1, select_value=None)
            vol.mask.zero(vol.stream)  # keep only the grown region
            L.check(lib.ivx_dev_flood_apply_where(vol.mask.ptr, vol.out_mask.ptr, c64(vol.n), 1, 255, vol.stream))
            out["region_grow"] = {"seeds": [list(s) for s in seeds], "rounds": rounds, "voxels": vol.reached_count()}
        if getattr(args, "crop", None) is not None:
            # the Crop mask tool (CropMaskInteractorStyle.CropMask, styles.py:2654-2694) on the resident mask
            with vol.timer.span("crop"):
                vol.crop_mask(args.crop)
            out["crop"] = {"limits": list(args.crop)}
        if getattr(args, "cut_polygon", None) or getattr(args, "brush3d", None):
            _mask3d_edit(args, vol, out)
        if args.mask_preview is not None:
            # "Mask 3D preview" (Mask.create_3d_preview -> VolumeMask.create_volume, volume_mask.py:36-119) of the resident mask
            from . import volume as V
            w, h = args.size
            with vol.timer.span("mask_preview"):
                rgba8 = vol.render_mask_preview(args.mask_colour, args.view, (w, h), mode=args.mask_preview, rgba8=True)
            out["mask_preview"] = {"mode": args.mask_preview, "colour": list(args.mask_colour), "view": args.view,
                                   "size": [w, h], **vol.last_render_stats}
            if args.png:
                V.write_png(args.png, rgba8)
                out["mask_preview"]["png"] = args.png
        if args.show_slice is not None:
            _show_slice(args, proj, vol, True, out)
        mask = vol.download_mask()
        out["mask_voxels"] = int(np.count_nonzero(mask >= 127))
        with vol.timer.span("surface"):
            nv, nt = vol.marching_cubes_indexed(from_binary=True, fill_border_holes=True)
        verts_buf, faces_buf = vol._verts, vol._faces
        _surface_tail(args, lib, out, verts_buf, faces_buf, nv, nt, vol.stream, vol.timer, vol.sync, (vol.shape, vol.spacing), vol, proj)
        if args.save:
            rec = prj.new_mask(proj, args.mask_name, (lo, hi))
            rec.matrix[1:, 1:, 1:] = mask
            if segmented:  # apply_segment_threshold's "fully edited" flag lines (segment.py:481-486)
                rec.matrix[:, 0, 0] = 2
                rec.matrix[0, :, 0] = 2
                rec.matrix[0, 0, :] = 2
            else:
                rec.matrix[1:, 0, 0] = 1  # per-slice "already thresholded" flags, as SetMaskThreshold leaves them (slice_.py:1246)
            if filtered is not None:
                img, ftype, fvalue, dimension, orientation = filtered
                label = prj.add_image_version(proj, img, ftype, fvalue, dimension, orientation)
                rec.derived_from = label  # _after_filter's create_new_mask(derived_from=label)
                out["image_version"] = label
            prj.save_inv3(args.save, proj)
            out["saved"] = args.save
        out["gpu_ms"] = {k: round(float(sum(v)), 4) for k, v in vol.timer.collect().items()}
    finally:
        vol.close()
        for b in bound:
            b.release()
        proj.close()
        out["wall_s"] = round(time.perf_counter() - t_all, 3)
    return out


def _surface_tail(args, lib, out, verts_buf, faces_buf, nv, nt, stream, timer, sync, geometry, vol=None, proj=None):
    """everything the driver does with a surface once it is resident (two device buffers, nv points, nt triangles): --largest,
    --surface-seed, --remove-nonvisible, --smooth, the measures, --stl, --surface-png, --scene-png, --geodesic, --split.  The
    surface comes from marching cubes on the mask or from --import-surface; `geometry`: the image's (shape, spacing) for the
    camera of --surface-png, or None without an image; `vol`, `proj`: the resident volume and the project of --scene-png"""
    out["surface"] = {"vertices": nv, "triangles": nt}
    keep_v = keep_f = None
    if args.largest and nt:
        from .device import DeviceBuffer
        keep_v, keep_f = DeviceBuffer(nv * 12 + 16), DeviceBuffer(nt * 12 + 16)
        n1, n2, nr = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        with timer.span("keep_largest"):
            L.check(lib.ivx_dev_mesh_keep_largest(verts_buf.ptr, c64(nv), faces_buf.ptr, c64(nt), keep_v.ptr, c64(nv),
                                                  keep_f.ptr, c64(nt), ctypes.byref(n1), ctypes.byref(n2),
                                                  ctypes.byref(nr), stream), "keep_largest")
        verts_buf, faces_buf, nv, nt = keep_v, keep_f, n1.value, n2.value
        out["largest"] = {"regions": nr.value, "vertices": nv, "triangles": nt}
    seeded = None
    if args.surface_seed and nt:
        # Surface.OnSeedSurface -> pu.JoinSeedsParts (surface.py:363-411): the GUI's point pick is the nearest point here
        from . import polydata_utils as pu
        whole = pu.DeviceMesh(verts_buf, nv, faces_buf, nt, stream)
        picks = [tuple(args.surface_seed[i:i + 3]) for i in range(0, len(args.surface_seed), 3)]
        with timer.span("surface_seed"):
            ids = [whole.nearest_point(xyz) for xyz in picks]
            seeded = whole.select_seeded(ids)
        out["surface_seed"] = {"points": [list(xyz) for xyz in picks], "point_ids": ids, "vertices": seeded.nverts,
                               "triangles": seeded.ntris}
        verts_buf, faces_buf, nv, nt = seeded.verts, seeded.faces, seeded.nverts, seeded.ntris
    shell = None
    if args.remove_nonvisible and nt:
        # Surface.OnRemoveNonVisibleFaces -> pu.RemoveNonVisibleFaces (surface.py:413-435) on the resident mesh
        from . import polydata_utils as pu
        with timer.span("remove_nonvisible"):
            shell = pu.RemoveNonVisibleFaces(pu.DeviceMesh(verts_buf, nv, faces_buf, nt, stream))
        out["remove_nonvisible"] = {"vertices": shell.nverts, "triangles": shell.ntris, "removed_triangles": nt - shell.ntris}
        verts_buf, faces_buf, nv, nt = shell.verts, shell.faces, shell.nverts, shell.ntris
    if args.smooth and nt:
        from .device import DeviceBuffer
        nrm = DeviceBuffer(nt * 24 + 16)
        with timer.span("smooth"):
            L.check(lib.ivx_dev_mesh_face_normals(verts_buf.ptr, L.F32, faces_buf.ptr, c64(nt), nrm.ptr, stream))
            L.check(lib.ivx_dev_context_aware_smoothing(verts_buf.ptr, L.F32, c64(nv), faces_buf.ptr, c64(nt), nrm.ptr,
                                                        ctypes.c_double(args.angle), ctypes.c_double(args.max_distance),
                                                        ctypes.c_double(args.min_weight), ctypes.c_int(args.steps), None,
                                                        None, stream), "ca_smoothing")
        nrm.close()
        out["smooth"] = {"angle": args.angle, "max_distance": args.max_distance, "min_weight": args.min_weight,
                         "steps": args.steps}
    from .device import DeviceBuffer
    mass = DeviceBuffer(64)
    with timer.span("mass"):
        L.check(lib.ivx_dev_mesh_mass_properties(verts_buf.ptr, faces_buf.ptr, c64(nt), mass.ptr, stream))
    sync()
    m = mass.download((8,), np.float64)
    out["volume"], out["area"] = float(m[0]), float(m[1])
    mass.close()
    verts = faces = None
    if args.stl:
        verts = verts_buf.download((nv, 3), np.float32)
        faces = faces_buf.download((nt, 3), np.int32)
        sp.write_stl_binary(args.stl, verts[faces])
        out["stl"] = args.stl
    if getattr(args, "surface_png", None):
        # the 3-D view's picture of the final surface (Surface._show_surface, surface.py:1061-1116, under the viewer's
        # camera of the IMAGE: the picture overlays --render), with the point normals the reference's actor carries
        from . import surface_view as SV
        from . import volume as V
        if verts is None:
            verts = verts_buf.download((nv, 3), np.float32)
            faces = faces_buf.download((nt, 3), np.int32)
        pv, pf, pn, _ = sp.point_normals(verts, faces)
        w, h = args.size
        actor = SV.SurfaceActor(pv, pf, pn, colour=args.surface_colour, transparency=args.surface_transparency)
        rgba8 = SV.render_surfaces([actor], args.view, (w, h), shape=geometry[0], spacing=geometry[1],
                                   interpolation=args.surface_interpolation, rgba8=True)
        V.write_png(args.surface_png, rgba8)
        out["surface_view"] = {"png": args.surface_png, "view": args.view, "size": [w, h], "colour": list(args.surface_colour),
                               "transparency": args.surface_transparency, "interpolation": args.surface_interpolation,
                               "vertices": int(len(pv)), "triangles": int(len(pf))}
    if getattr(args, "scene_png", None):
        # the 3-D view with everything the run has in it: the ray-cast image of --render or the mask of
        # --mask-preview composite, the final surface with the --surface-* options, and the slice planes of --slice-planes under
        # --window, every fragment blended at its depth
        from . import scene3d as S3
        from . import surface_view as SV
        from . import volume as V
        if verts is None:
            verts = verts_buf.download((nv, 3), np.float32)
            faces = faces_buf.download((nt, 3), np.int32)
        pv, pf, pn, _ = sp.point_normals(verts, faces)
        w, h = args.size
        actor = SV.SurfaceActor(pv, pf, pn, colour=args.surface_colour, transparency=args.surface_transparency)
        planes = [S3.SlicePlane(o, n) for o, n in zip(("AXIAL", "CORONAL", "SAGITAL"), args.slice_planes or ()) if n >= 0]
        field = {}
        if args.render is not None:
            pdir = args.presets_dir
            if pdir is None and args.render.endswith(".plist"):
                pdir = os.path.dirname(os.path.abspath(args.render))
            field = {"preset": args.render, "presets_dir": pdir}
        elif args.mask_preview is not None:
            field = {"mask_colour": args.mask_colour}
        with S3.Scene3D(vol, [actor] if len(pf) else None, planes) as scene:
            with timer.span("scene"):
                rgba8 = scene.render(args.view, (w, h), interpolation=args.surface_interpolation, rgba8=True,
                                     state=display_state(args, proj) if planes else None, **field)
            stats = scene.last_render_stats
        V.write_png(args.scene_png, rgba8)
        out["scene"] = {"png": args.scene_png, "view": args.view, "size": [w, h], "field": "image" if args.render is not None else
                        ("mask" if args.mask_preview is not None else None), "triangles": int(len(pf)),
                        "planes": {p.orientation: p.n for p in planes}, **stats}
    if args.geodesic:
        # the measurement panel's geodesic measure (GeodesicMeasure._draw_line, measures.py:1202-1256) on the final surface
        from . import polydata_utils as pu
        picks = [tuple(args.geodesic[i:i + 3]) for i in range(0, len(args.geodesic), 3)]
        final = pu.DeviceMesh(verts_buf, nv, faces_buf, nt, stream)
        try:
            with timer.span("geodesic"):
                geo = final.geodesic(points=picks)
        finally:
            final.close()  # (frees the graph; the buffers are not its own)
        out["geodesic"] = {"points": [list(xyz) for xyz in picks], "point_ids": [int(i) for i in geo.point_ids],
                           "segment_lengths": geo.segment_lengths, "length_mm": geo.length, "path_points": len(geo.points)}
        if args.geodesic_npy:
            np.save(args.geodesic_npy, geo.points)
            out["geodesic"]["npy"] = args.geodesic_npy
    if args.split is not None:
        # Surface.OnSplitSurface -> pu.SplitDisconectedParts (surface.py:319-361) on the final surface: one STL per part, in
        # region order, and every part's measures (CreateSurfaceFromPolydata takes them per part, surface.py:953-960)
        from . import polydata_utils as pu
        os.makedirs(args.split, exist_ok=True)
        with timer.span("split"):
            parts = pu.DeviceMesh(verts_buf, nv, faces_buf, nt, stream).split()
            measures = parts.mass_properties()
        table = parts.table
        rows = []
        for r in range(parts.n):
            if int(table[r, 1]) < args.split_min_triangles:
                continue
            pv, pf = parts.download(r)
            name = os.path.join(args.split, "part_%05d.stl" % r)
            sp.write_stl_binary(name, pv[pf])
            rows.append({"part": r, "triangles": int(table[r, 1]), "vertices": int(table[r, 3]), "volume": float(measures[r, 0]),
                         "area": float(measures[r, 1]), "stl": name})
        parts.close()
        out["split"] = {"regions": parts.n, "min_triangles": args.split_min_triangles, "parts": rows}
    for b in (keep_v, keep_f):
        if b is not None:
            b.close()
    if shell is not None:
        shell.close()
    if seeded is not None:
        seeded.close()


def run_import(args) -> dict:
    """--import-surface FILE: Surface.OnImportSurfaceFile (surface.py:619-845) -- the file's mesh, welded on the GPU where the
    format holds a soup, takes the place of the marching-cubes surface; --import-world converts it from world to InVesalius
    coordinates with the project's affine, spacing and shape first (ConvertPolydataToInv).  No image is opened otherwise."""
    from . import surface as S
    from .device import Timer

    t_all = time.perf_counter()
    out, convert, geometry = {}, None, None
    if args.project is not None:
        proj = prj.open_inv3(args.project)
        try:
            out.update({"project": proj.name, "shape": list(proj.matrix_shape), "spacing": list(proj.spacing)})
            geometry = (tuple(proj.matrix_shape), tuple(proj.spacing))
            if args.import_world:
                affine = np.eye(4) if proj.affine is None else np.array(proj.affine, np.float64).reshape(4, 4)
                convert = (affine, proj.spacing, proj.matrix_shape)
        finally:
            proj.close()
    lib = L.lib()
    imp = S.CreateSurfaceFromFile(args.import_surface, convert_to_inv=convert)
    mesh, timer = imp.mesh, Timer(None)
    try:
        c = imp.counts
        out["import"] = {"file": args.import_surface, "name": imp.name, "format": imp.format, "facets_read": c["facets_read"],
                         "vertices": mesh.nverts, "triangles": mesh.ntris, "dropped": c["dropped"], "volume": imp.volume,
                         "area": imp.area, "world": bool(args.import_world)}
        _surface_tail(args, lib, out, mesh.verts, mesh.faces, mesh.nverts, mesh.ntris, mesh.stream, timer, mesh.sync, geometry)
        mesh.sync()
        out["gpu_ms"] = {k: round(float(sum(v)), 4) for k, v in timer.collect().items()}
    finally:
        imp.close()
        out["wall_s"] = round(time.perf_counter() - t_all, 3)
    return out


def _image_geometry(args, proj, bound, out):
    """--flip, --swap-axes, --gantry-tilt, in that order, on the project's bound image before anything else (Slice.OnFlipVolume,
    Slice.OnSwapVolumeAxes, imagedata_utils.FixGantryTilt): the image versions follow, every mask of the project is cleared
    (or recreated at the new shape), and the project records the new shape and spacing the way the reference updates
    ``matrix_shape`` and ``spacing`` (slice_.py:2198-2200), so --save writes them."""
    from . import slice_ as sl

    flip, swap, tilt = getattr(args, "flip", None), getattr(args, "swap_axes", None), getattr(args, "gantry_tilt", None)
    if flip is None and swap is None and tilt is None:
        return
    masks = list(proj.masks.values())
    if flip is not None:
        sl.flip_volume(proj.matrix, flip, masks=masks, versions=proj.image_versions)
        out["flip"] = int(flip)
    if swap is not None:
        labels = [label for label, mat in proj.image_versions if mat is not proj.matrix]
        new, spacing, _, versions = sl.swap_volume_axes(proj.matrix, swap, proj.spacing, masks=masks, versions=proj.image_versions)
        swapped = dict(zip(labels, versions))
        proj.image_versions = [(label, swapped.get(label, new)) for label, _ in proj.image_versions]
        proj.matrix, proj.matrix_shape, proj.spacing = new, tuple(new.shape), tuple(spacing)
        bound[0] = resident.find(new)
        out["swap_axes"] = [int(v) for v in swap]
    if tilt is not None:
        sl.fix_gantry_tilt(proj.matrix, proj.spacing, tilt, masks=masks)
        out["gantry_tilt"] = float(tilt)
    out["shape"], out["spacing"] = list(proj.matrix.shape), list(proj.spacing)


SHOW_PROJECTIONS = {"normal": 0, "maxip": 1, "minip": 2, "meanip": 3, "mida": 5, "contour_mip": 6, "contour_lmip": 7, "contour_mida": 8}


def display_state(args, proj):
    """the DisplayState of --show-slice: --window (default: the project's), --colour-table (one of const.SLICE_COLOR_TABLE,
    or a colour list of --presets-dir, shown like the reference's PLIST mode), --mask-colour at the default mask opacity"""
    from . import slice_display as D
    from . import volume as V

    ww, wl = args.window if args.window is not None else (proj.window, proj.level)
    st = D.DisplayState(window_width=float(ww), window_level=float(wl), mask_colour=tuple(args.mask_colour))
    name = args.colour_table
    if name is not None:
        tables = {k.strip().lower(): k for k in D.SLICE_COLOR_TABLE}
        if name.strip().lower() in tables:
            st.set_colour_table(tables[name.strip().lower()])
        elif args.presets_dir is None:
            raise KeyError("--colour-table %r is none of %s: a colour list needs --presets-dir DIR" % (name, sorted(tables.values())))
        else:
            st.set_plist(np.asarray(V.load_color_list(name, args.presets_dir)).astype(np.int64))
    return st


def _show_slice(args, proj, vol, with_mask, out):
    """--show-slice: Slice.GetSlices (slice_.py:746-830) of one slice -- or of a slab's projection, computed from the bound
    image and handed over on the device -- with the resident mask drawn over it; written as a PNG (alpha 255)"""
    from . import slice_ as sl
    from . import volume as V
    from .device import DeviceBuffer

    ori, n = args.show_slice[0].upper(), int(args.show_slice[1])
    st = display_state(args, proj)
    tp = SHOW_PROJECTIONS[args.projection]
    block, dtype = None, np.int16
    with vol.timer.span("show_slice"):
        if tp != sl.PROJECTION_NORMAL:
            image = sl.get_image_slice(proj.matrix, ori, n, args.slab, False, 1.0, tp, st.window_level)
            block, dtype = DeviceBuffer(image.nbytes), image.dtype
            block.upload(image)
        rgb = vol.show_slice(ori, n, st, image=block, image_dtype=dtype, mask=with_mask)
    if block is not None:
        block.close()
    out["show_slice"] = {"orientation": ori, "slice": n, "window": [st.window_width, st.window_level], "colour_table": args.colour_table,
                         "projection": args.projection, "slab": args.slab if tp else 1, "mask": bool(with_mask), "size": [rgb.shape[1], rgb.shape[0]]}
    if args.png:
        V.write_png(args.png, np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2))
        out["show_slice"]["png"] = args.png


def _measures_asked(args) -> bool:
    return bool(getattr(args, "density_ellipse", None) or getattr(args, "density_polygon", None) or getattr(args, "remeasure", False))


def _density(args, proj, vol, out):
    """--density-ellipse / --density-polygon / --remeasure: the measurement panel's density measures (DensityMeasureEllipseStyle,
    DensityMeasurePolygonStyle, styles.py:1023-1166; calc_density, measures.py:2019-2107, 2229-2319) on the resident image
    (after --filter), all of them in one launch.  --remeasure first recomputes every density entry the project holds; the new
    measures are appended to ``project.measurements`` under ``str(index)``, index = len(dict), as Project.AddMeasurement does
    (project.py:173-177), so --save writes them."""
    from . import measures as M

    block = {}
    with vol.timer.span("density"):
        if getattr(args, "remeasure", False):
            block["remeasured"] = M.recompute_measurements(proj.measurements, vol, proj.spacing)
        new = []
        for spec in getattr(args, "density_ellipse", None) or []:
            c = [float(v) for v in spec[2:]]
            new.append((M.CircleDensityMeasure(spec[0].upper(), int(spec[1]), tuple(c[0:3]), tuple(c[3:6]), tuple(c[6:9])), M.DENSITY_ELLIPSE))
        for spec in getattr(args, "density_polygon", None) or []:
            c = [float(v) for v in spec[2:]]
            new.append((M.PolygonDensityMeasure(spec[0].upper(), int(spec[1]), [tuple(c[i:i + 3]) for i in range(0, len(c), 3)]), M.DENSITY_POLYGON))
        for m, kind in new:
            dm = M.DensityMeasurement()
            dm.location, dm.type, dm.slice_number = M.LOCATIONS[m.orientation], kind, m.slice_number
            m.set_measurement(dm)
        results = M.density_of(vol, proj.spacing, [m for m, _ in new])
        for m, _ in new:
            dm = m._measurement
            dm.index = len(proj.measurements)
            dm.name = M.MEASURE_NAME_PATTERN % (dm.index + 1)
            dm.points = [list(p) for p in dm.points]
            proj.measurements[str(dm.index)] = dm.get_as_dict()
    block["measures"] = [{"orientation": m.orientation, "slice": m.slice_number, "type": kind, "index": m._measurement.index, **r}
                         for (m, kind), r in zip(new, results)]
    out["density"] = block
    if getattr(args, "measures_json", None):
        with open(args.measures_json, "w") as f:
            json.dump({"measures": block["measures"], "measurements": proj.measurements}, f)
        out["density"]["json"] = args.measures_json


def _measure_only(args) -> bool:
    """the density flags without anything that asks for a mask, a surface or a picture: the numbers (and --save) are all"""
    return (args.threshold is None and args.segment is None and not args.seed and not args.stl and not args.largest and not args.smooth
            and not args.remove_nonvisible and not args.surface_seed and args.split is None and not getattr(args, "geodesic", None)
            and getattr(args, "crop", None) is None and not getattr(args, "surface_png", None) and not getattr(args, "scene_png", None)
            and args.render is None
            and args.mask_preview is None and args.show_slice is None and "--mask" not in (args.argv or []))


def _show_only(args) -> bool:
    """--show-slice without --threshold, --mask or --segment: there is no mask to draw"""
    return args.threshold is None and args.segment is None and "--mask" not in (args.argv or [])


def _render_only(args) -> bool:
    """--render without anything that asks for a mask or a surface: the image is all there is to make"""
    return (args.threshold is None and args.segment is None and not args.seed and not args.stl and not args.save
            and not args.largest and not args.smooth and not args.remove_nonvisible and not args.surface_seed
            and args.split is None and not getattr(args, "geodesic", None) and getattr(args, "crop", None) is None
            and not getattr(args, "surface_png", None) and not getattr(args, "scene_png", None) and "--mask" not in (args.argv or []))


def _strct(conn: int) -> np.ndarray:
    from .mask import CON3D, _structure
    return _structure(3, CON3D[conn])


def parse_cut_polygon(values):
    """--cut-polygon MODE DEPTH X Y X Y ...: (edit mode, depth value 0..1, (N, 2) display points)"""
    if len(values) < 4 or len(values) % 2:
        raise ValueError("--cut-polygon takes MODE DEPTH and then X Y pairs")
    mode, depth = int(values[0]), float(values[1])
    if mode not in (0, 1):
        raise ValueError("--cut-polygon MODE is 0 (include) or 1 (exclude)")
    return mode, depth, np.array([float(v) for v in values[2:]], np.float64).reshape(-1, 2)


def parse_brush3d(values):
    """--brush3d MODE SIZE X Y Z ...: (edit mode, brush size, (N, 3) world points)"""
    if len(values) < 5 or (len(values) - 2) % 3:
        raise ValueError("--brush3d takes MODE SIZE and then X Y Z triples")
    mode = int(values[0])
    if mode not in (0, 1):
        raise ValueError("--brush3d MODE is 0 (include) or 1 (exclude)")
    return mode, float(values[1]), np.array([float(v) for v in values[2:]], np.float64).reshape(-1, 3)


def _mask3d_edit(args, vol, out):
    """the 3-D mask editor (Mask3DEditorState.CutMaskFromPolygons / brush_stroke, mask3d_editor_state.py) on the resident mask:
    every --cut-polygon is one completed polygon cut through the --view camera of a --cut-size viewport, down to
    near + (far - near) * DEPTH; every --brush3d is one drag"""
    from . import mask3d_editor as M3
    from . import volume as V

    if args.cut_polygon:
        w, h = args.cut_size
        cam = V.resolve_camera(args.view, vol.shape, vol.spacing, (w, h))
        near, far = M3.default_clipping_range(cam)
        m, mv = M3.camera_matrices(cam, (w, h), (near, far))
        out["cut_polygon"] = []
        for values in args.cut_polygon:
            mode, depth, pts = parse_cut_polygon(values)
            with vol.timer.span("cut_polygon"):
                flags = vol.cut_mask([pts], (w, h), m, mv, near + (far - near) * depth, mode)
            out["cut_polygon"].append({"mode": mode, "depth": depth, "points": len(pts), "size": [w, h], "view": args.view,
                                       "slices_changed": int(flags.sum())})
    if args.brush3d:
        out["brush3d"] = []
        for values in args.brush3d:
            mode, size, pts = parse_brush3d(values)
            with vol.timer.span("brush3d"):
                flags = vol.brush_mask_stroke(pts, size, mode)
            out["brush3d"].append({"mode": mode, "size": size, "dabs": len(pts), "slices_changed": int(flags.sum())})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m invesalius3_amd.headless", description=__doc__.split("\n")[0])
    ap.add_argument("project", nargs="?", default=None, help=".inv3 file (may be left out with --import-surface)")
    ap.add_argument("--import-surface", metavar="FILE", default=None,
                    help="import a surface file (.stl, .ply, .vtp) instead of making one from a mask: --largest, --remove-nonvisible, "
                         "--surface-seed, --split, --smooth, --geodesic and --stl act on it; not with --threshold or --segment")
    ap.add_argument("--import-world", action="store_true",
                    help="convert the imported surface from world to InVesalius coordinates with the project's affine, spacing and shape")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--threshold", nargs=2, type=int, metavar=("LO", "HI"), help="threshold the image into a new mask")
    g.add_argument("--mask", type=int, default=0, help="use the project's mask with this index (default 0)")
    g.add_argument("--segment", choices=("brain", "trachea"), default=None,
                   help="deep-learning segmentation into a new mask (Brain MRI T1 / Trachea CT); needs --weights")
    ap.add_argument("--weights", default=None, help="the tool's torch.save weights file (brain_mri_t1.pt / trachea_ct.pt) "
                                                   "or an .npz of the same keys; never downloaded")
    ap.add_argument("--seg-threshold", type=float, default=0.75, help="probability threshold of --segment (default 0.75)")
    ap.add_argument("--overlap", type=int, choices=(0, 10, 25, 50), default=50, help="patch overlap in %% (default 50)")
    ap.add_argument("--apply-wwwl", nargs=2, type=float, metavar=("WW", "WL"), default=None,
                    help="window the image (get_LUT_value) before --segment")
    ap.add_argument("--seed", nargs="+", type=int, default=None, metavar="X Y Z", help="keep the region grown (in the image, inside the threshold range) from these voxels; refused for a hand-edited --mask")
    ap.add_argument("--crop", nargs=6, type=int, default=None, metavar=("XI", "XF", "YI", "YF", "ZI", "ZF"),
                    help="crop the mask to this box of voxel limits (the Crop mask tool), after --threshold and --seed")
    ap.add_argument("--cut-polygon", nargs="+", action="append", default=None, metavar="MODE DEPTH X Y",
                    help="cut the mask with a polygon of display points drawn on the --view camera's --cut-size viewport (the 3-D mask "
                         "editor): MODE 0 keeps what is inside, 1 removes it; DEPTH 0..1 of the clipping range; repeatable; after "
                         "--threshold, --seed and --crop")
    ap.add_argument("--cut-size", nargs=2, type=int, metavar=("W", "H"), default=(512, 512), help="viewport of --cut-polygon (default 512 512)")
    ap.add_argument("--brush3d", nargs="+", action="append", default=None, metavar="MODE SIZE X Y Z",
                    help="a drag of the 3-D brush through these world points: MODE 1 erases, 0 paints 255; SIZE the diameter; repeatable")
    ap.add_argument("--flip", type=int, choices=(0, 1, 2), default=None, metavar="AXIS",
                    help="flip the image along axis 0 (z), 1 (y) or 2 (x) first (the Flip tool); masks are cleared")
    ap.add_argument("--swap-axes", nargs=2, type=int, default=None, metavar=("A", "B"),
                    help="then swap two axes of the image (the Swap axes tool): new shape and spacing; masks are recreated")
    ap.add_argument("--gantry-tilt", type=float, default=None, metavar="DEGREES",
                    help="then correct a gantry tilt of this many degrees (FixGantryTilt), before any segmentation")
    ap.add_argument("--filter", nargs=2, metavar=("NAME", "VALUE"), default=None,
                    help="image filter applied before --threshold / --seed: NAME one of %s, VALUE the dialog's value "
                         "(sigma, or the size parameter)" % ",".join(FILTER_TYPES))
    ap.add_argument("--filter-2d", choices=("axial", "coronal", "sagittal"), default=None,
                    help="filter slice by slice along this orientation instead of in 3-D")
    ap.add_argument("--render", metavar="PRESET", default=None,
                    help="volume-render the image (after --filter) with a raycasting preset: a .plist file, or a preset "
                         "name looked up in --presets-dir")
    ap.add_argument("--mask-preview", choices=("composite", "iso"), default=None,
                    help="ray-cast the mask (after --threshold / --seed / --segment, or the project's --mask) as a shaded solid: "
                         "the reference's Mask 3D preview with rendering 0 (composite) or 1 (iso-surface at 127)")
    ap.add_argument("--mask-colour", nargs=3, type=float, metavar=("R", "G", "B"), default=(0.0, 1.0, 0.0),
                    help="the mask's colour, 0..1 each (default 0 1 0)")
    ap.add_argument("--show-slice", nargs=2, metavar=("ORIENTATION", "N"), default=None,
                    help="the slice viewer's picture of slice N (AXIAL, CORONAL or SAGITAL): window/level, colour table and the "
                         "mask's overlay when --threshold or --mask is given; written to --png")
    ap.add_argument("--window", nargs=2, type=float, metavar=("WW", "WL"), default=None, help="window width and level of --show-slice (default: the project's)")
    ap.add_argument("--colour-table", metavar="NAME", default=None,
                    help="colour table of --show-slice: Default, Hue, Saturation, Desert, Rainbow, Ocean, Inverse Gray, or a colour list of --presets-dir")
    ap.add_argument("--projection", choices=tuple(SHOW_PROJECTIONS), default="normal", help="--show-slice shows this projection of a slab of --slab slices")
    ap.add_argument("--slab", type=int, default=1, metavar="K", help="slices in the projected slab (default 1)")
    ap.add_argument("--presets-dir", metavar="DIR", default=None, help="the raycasting presets directory (with color_list/)")
    ap.add_argument("--view", choices=("front", "back", "left", "right", "top", "bottom", "iso"), default="iso")
    ap.add_argument("--size", nargs=2, type=int, metavar=("W", "H"), default=(512, 512), help="image size (default 512 512)")
    ap.add_argument("--png", metavar="OUT", default=None, help="write the rendered image as an RGBA PNG")
    ap.add_argument("--connectivity", type=int, choices=(6, 18, 26), default=26)
    gs = ap.add_mutually_exclusive_group()
    gs.add_argument("--largest", action="store_true", help="keep the largest connected surface")
    gs.add_argument("--surface-seed", nargs="+", type=float, default=None, metavar="X Y Z",
                    help="keep the connected parts of the surface that hold the points nearest to these coordinates (the "
                         "reference's Select regions of interest); not with --largest")
    ap.add_argument("--split", metavar="DIR", default=None,
                    help="split the final surface into its connected parts: DIR/part_%%05d.stl per part, in region order, and "
                         "a table of triangles, volume and area in the JSON line")
    ap.add_argument("--split-min-triangles", type=int, default=1, metavar="N",
                    help="leave parts with fewer than N triangles out of --split's files and table (default 1)")
    ap.add_argument("--geodesic", nargs="+", type=float, default=None, metavar="X Y Z",
                    help="the geodesic measure on the final surface: the shortest path along the triangle edges through the "
                         "mesh points nearest to these two or more coordinates, its length in mm in the JSON line")
    ap.add_argument("--geodesic-npy", metavar="FILE", default=None, help="write the path's coordinates, float32 (n, 3), as .npy")
    ap.add_argument("--remove-nonvisible", action="store_true",
                    help="remove the faces that cannot be seen from outside (the six axis views at 800 x 800 of the reference's "
                         "Remove non-visible faces), after --largest and before --smooth / --stl")
    ap.add_argument("--smooth", action="store_true", help="context-aware smoothing")
    ap.add_argument("--angle", type=float, default=0.7)
    ap.add_argument("--max-distance", type=float, default=3.0)
    ap.add_argument("--min-weight", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--stl", help="write the surface as binary STL")
    ap.add_argument("--surface-png", metavar="OUT", default=None,
                    help="write a shaded picture of the final surface (after --largest / --surface-seed / --remove-nonvisible / "
                         "--smooth) as an RGBA PNG, from --view at --size with the camera of the image: it overlays --render")
    ap.add_argument("--scene-png", metavar="OUT", default=None,
                    help="write the 3-D view with everything in it as an RGBA PNG: the image of --render or the mask of --mask-preview "
                         "composite, the final surface (--surface-colour, --surface-transparency, --surface-interpolation) and the "
                         "planes of --slice-planes, each blended at its depth (--view, --size)")
    ap.add_argument("--slice-planes", nargs=3, type=int, metavar=("AXIAL_N", "CORONAL_N", "SAGITAL_N"), default=None,
                    help="the slice planes of --scene-png at these slice numbers (-1: off), shown under --window")
    ap.add_argument("--surface-colour", nargs=3, type=float, metavar=("R", "G", "B"), default=(0.33, 1.0, 0.33),
                    help="the surface's colour, 0..1 each (default: the reference's first surface colour)")
    ap.add_argument("--surface-transparency", type=float, default=0.0, metavar="T", help="the surface's transparency, 0..1 (default 0)")
    ap.add_argument("--surface-interpolation", choices=("flat", "gouraud", "phong"), default="gouraud",
                    help="shading of --surface-png (default gouraud, the reference's default)")
    ap.add_argument("--density-ellipse", nargs=11, action="append", default=None,
                    metavar=("ORIENTATION", "N", "CX", "CY", "CZ", "P1X", "P1Y", "P1Z", "P2X", "P2Y", "P2Z"),
                    help="the ellipse density measure on slice N (AXIAL, CORONAL or SAGITAL): centre and the two handle points in mm; "
                         "min, max, mean, std, area and perimeter in the JSON line; repeatable")
    ap.add_argument("--density-polygon", nargs="+", action="append", default=None, metavar="ORIENTATION N X Y Z",
                    help="the polygon density measure on slice N through three or more points x y z in mm; repeatable")
    ap.add_argument("--remeasure", action="store_true", help="recompute every density measure the project holds from the image")
    ap.add_argument("--measures-json", metavar="FILE", default=None, help="write the measures' results and the project's measurements as JSON")
    ap.add_argument("--save", help="write the project back with the new mask (and the new measures) appended")
    ap.add_argument("--mask-name", default="GPU mask")
    args = ap.parse_args(argv)
    args.argv = list(sys.argv[1:] if argv is None else argv)
    if args.import_surface is not None:
        if args.threshold is not None or args.segment is not None or "--mask" in args.argv or args.seed:
            ap.error("--import-surface takes the place of --threshold / --segment / --mask / --seed: name one source of the surface")
        image_flags = ("filter", "render", "mask_preview", "show_slice", "save", "crop", "cut_polygon", "brush3d", "flip", "swap_axes",
                       "gantry_tilt", "density_ellipse", "density_polygon", "remeasure", "scene_png")
        given = [f for f in image_flags if getattr(args, f, None)]
        if given:
            ap.error("--import-surface works on the surface alone: --%s needs the image or the mask" % given[0].replace("_", "-"))
        if args.geodesic_npy is not None and args.geodesic is None:
            ap.error("--geodesic-npy needs --geodesic")
        if args.import_world and args.project is None:
            ap.error("--import-world needs the project whose affine, spacing and shape it uses")
        if args.surface_png is not None and args.project is None:
            ap.error("--surface-png of an imported surface needs the project whose image sets the camera")
        if args.geodesic is not None and (len(args.geodesic) < 6 or len(args.geodesic) % 3):
            ap.error("--geodesic takes two or more triples of x y z")
        if args.surface_seed and len(args.surface_seed) % 3:
            ap.error("--surface-seed takes triples of x y z")
        print(json.dumps(run_import(args)))
        return 0
    if args.project is None:
        ap.error("the following arguments are required: project")
    if args.import_world:
        ap.error("--import-world needs --import-surface FILE")
    if args.segment is not None:
        if args.weights is None:
            ap.error("--segment needs --weights FILE")
        if args.seed:
            ap.error("--seed does not combine with --segment")
    elif args.weights is not None or args.apply_wwwl is not None:
        ap.error("--weights / --apply-wwwl need --segment")
    if args.seed and len(args.seed) % 3:
        ap.error("--seed takes triples of x y z")
    if args.surface_seed and len(args.surface_seed) % 3:
        ap.error("--surface-seed takes triples of x y z")
    if args.geodesic is not None and (len(args.geodesic) < 6 or len(args.geodesic) % 3):
        ap.error("--geodesic takes two or more triples of x y z")
    if args.geodesic_npy is not None and args.geodesic is None:
        ap.error("--geodesic-npy needs --geodesic")
    for spec in (args.density_ellipse or []) + (args.density_polygon or []):
        if spec[0].upper() not in ("AXIAL", "CORONAL", "SAGITAL") or len(spec) < 2 or not spec[1].lstrip("-").isdigit():
            ap.error("--density-ellipse / --density-polygon take AXIAL, CORONAL or SAGITAL and a slice number first")
        try:
            [float(v) for v in spec[2:]]
        except ValueError:
            ap.error("--density-ellipse / --density-polygon take coordinates in mm")
    for spec in args.density_polygon or []:
        if len(spec) < 5 or (len(spec) - 2) % 3:
            ap.error("--density-polygon takes ORIENTATION N and triples of x y z")
    if args.measures_json is not None and not _measures_asked(args):
        ap.error("--measures-json needs --density-ellipse, --density-polygon or --remeasure")
    if args.split_min_triangles != 1 and args.split is None:
        ap.error("--split-min-triangles needs --split DIR")
    if args.filter is not None:
        if args.filter[0] not in FILTER_TYPES:
            ap.error("--filter NAME must be one of %s" % ", ".join(FILTER_TYPES))
        try:
            float(args.filter[1])
        except ValueError:
            ap.error("--filter VALUE must be a number")
    elif args.filter_2d is not None:
        ap.error("--filter-2d needs --filter")
    if args.render is not None:
        if not args.render.endswith(".plist") and args.presets_dir is None:
            ap.error("--render NAME needs --presets-dir DIR (or give the .plist file)")
        if args.size[0] <= 0 or args.size[1] <= 0:
            ap.error("--size W H must be positive")
        if args.mask_preview is not None:
            ap.error("--render and --mask-preview make one picture each: name one of them")
    elif args.mask_preview is not None:
        if args.size[0] <= 0 or args.size[1] <= 0:
            ap.error("--size W H must be positive")
        if not all(0.0 <= c <= 1.0 for c in args.mask_colour):
            ap.error("--mask-colour R G B must lie in 0..1")
    elif args.png is not None and args.show_slice is None:
        ap.error("--png needs --render, --mask-preview or --show-slice")
    if args.surface_png is not None:
        if args.size[0] <= 0 or args.size[1] <= 0:
            ap.error("--size W H must be positive")
        if not all(0.0 <= c <= 1.0 for c in args.surface_colour) or not 0.0 <= args.surface_transparency <= 1.0:
            ap.error("--surface-colour R G B and --surface-transparency T must lie in 0..1")
    if args.scene_png is not None:
        if args.project is None:
            ap.error("--scene-png needs a project: the scene is seen with the camera of its image")
        if args.size[0] <= 0 or args.size[1] <= 0:
            ap.error("--size W H must be positive")
        if args.mask_preview == "iso":
            ap.error("--scene-png composes the composite mask preview (--mask-preview composite), not the iso mode")
        if not all(0.0 <= c <= 1.0 for c in args.surface_colour) or not 0.0 <= args.surface_transparency <= 1.0:
            ap.error("--surface-colour R G B and --surface-transparency T must lie in 0..1")
        if args.window is not None and not args.window[0] > 0:
            ap.error("--window WW WL: the width must be positive")
    elif args.slice_planes is not None:
        ap.error("--slice-planes needs --scene-png")
    if args.show_slice is not None:
        if args.show_slice[0].upper() not in ("AXIAL", "CORONAL", "SAGITAL") or not args.show_slice[1].lstrip("-").isdigit():
            ap.error("--show-slice takes AXIAL, CORONAL or SAGITAL and a slice number")
        if args.render is not None or args.mask_preview is not None:
            ap.error("--show-slice, --render and --mask-preview make one picture each: name one of them")
        if args.slab < 1:
            ap.error("--slab K must be positive")
        if args.window is not None and not args.window[0] > 0:
            ap.error("--window WW WL: the width must be positive")
    elif (args.window is not None and args.slice_planes is None) or args.colour_table is not None or args.projection != "normal" or args.slab != 1:
        ap.error("--window, --colour-table, --projection and --slab need --show-slice (--window also serves --slice-planes)")
    print(json.dumps(run(args)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
