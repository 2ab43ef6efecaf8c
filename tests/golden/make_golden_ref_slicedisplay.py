"""Golden numbers from the REFERENCE ITSELF for the slice display: everything its own Python decides around the VTK
filters of Slice.GetSlices (invesalius/data/slice_.py:746-830).  VTK's arithmetic is not recorded (it is not installed; rules
R1 - R7 are the project's statement of it).  The reference's modules are imported from its checkout (INVESALIUS_REFERENCE)
under the stand-in finder and the methods called unbound on plain namespaces.

    INVESALIUS_REFERENCE=<the reference's checkout> python3 tests/golden/make_golden_ref_slicedisplay.py

Recorded: const.SLICE_COLOR_TABLE, THRESHOLD_HUE_RANGE, MASK_OPACITY, MASK_COLOUR; presets.get_wwwl_preset_colours of every
color_list plist; the table range get_LUT_value_255((min, max), ww, wl) of do_colour_image; _update_wwwl_widget_nodes;
the window / level UpdateColourTableBackgroundWidget derives from nodes; the two colour dicts GetSlices hands
do_custom_colour (captured from a call of GetSlices); get_aux_slice.  Arrays and names only.
"""
import glob
import os
import sys
import tempfile
import types
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ref_dowatershed as M  # noqa: E402

RANGES = [(-1024, 3071, 255, 127), (-1024, 3071, 2000, 300), (-1024, 3071, 1, 0), (-1024, 3071, 65535, 0), (0, 255, 255.5, 127),
          (-32768, 32767, 400, 40), (5, 5, 100, 5), (-1024, 3071, 2, -32768), (-1024, 3071, 80, 32767), (100, 4000, 350, 50),
          (-2000, -1500, 1500, -600), (0, 1, 256, 128)]
NODE_SETS = [[(-200.0, (0, 0, 0)), (600.0, (255, 255, 255))],
             [(-1000.0, (0, 0, 255)), (0.5, (0, 255, 0)), (1500.25, (255, 0, 0))],
             [(float(30 * k - 100 + (k == 7) * -30), ((17 * k) % 256, (91 * k) % 256, (201 * k) % 256)) for k in range(16)]]
WWWL = [(255.0, 127.0), (2000.0, 300.0), (80.5, -40.25), (1.0, 3000.0)]


def main(path):
    tmp_root = tempfile.mkdtemp(prefix="ref_slicedisplay_")
    tempfile.tempdir = tmp_root
    os.environ["HOME"] = tmp_root
    sys.meta_path.insert(0, M._Finder())
    import pubsub.pub
    pubsub.pub.subscribe = lambda *a, **k: (None, True)
    pubsub.pub.sendMessage = lambda *a, **k: None
    reference = os.environ.get("INVESALIUS_REFERENCE")
    if not reference or not os.path.isdir(os.path.join(reference, "invesalius")):
        raise SystemExit("set INVESALIUS_REFERENCE to the reference's checkout (the directory that holds invesalius/)")
    sys.path.insert(0, reference)
    from invesalius import constants as const
    from invesalius import presets
    from invesalius.data import imagedata_utils as iu
    from invesalius.data import slice_ as rs
    rs.Publisher.sendMessage = lambda *a, **k: None

    d = {}
    names = list(const.SLICE_COLOR_TABLE)
    d["colour_table_names"] = np.array(names)
    d["colour_table_ncolours"] = np.array([-1 if const.SLICE_COLOR_TABLE[n][0] is None else const.SLICE_COLOR_TABLE[n][0] for n in names])
    d["colour_table_ranges"] = np.array([const.SLICE_COLOR_TABLE[n][1:] for n in names], np.float64)  # saturation, hue, value
    d["threshold_hue_range"] = np.array(const.THRESHOLD_HUE_RANGE, np.float64)
    d["mask_opacity"] = np.float64(const.MASK_OPACITY)
    d["mask_colour"] = np.array(const.MASK_COLOUR, np.float64)
    d["modes"] = np.array([rs.OTHER, rs.PLIST, rs.WIDGET])

    files = sorted(glob.glob(os.path.join(reference, "presets", "raycasting", "color_list", "*.plist")))
    d["plist_names"] = np.array([os.path.splitext(os.path.basename(f))[0] for f in files])
    for k, f in enumerate(files):
        d["plist_%d" % k] = np.array(presets.get_wwwl_preset_colours(f), np.int64)

    # do_colour_image's table range: int16 (min, max), as ``self.matrix.min()`` of the int16 image gives them
    d["range_cases"] = np.array(RANGES, np.float64)
    d["range_out"] = np.array([iu.get_LUT_value_255(np.array((np.int16(a), np.int16(b))), ww, wl) for a, b, ww, wl in RANGES], np.float64)

    # the CLUT widget's nodes under a window / level drag, and the window they imply
    from invesalius.gui.widgets.clut_imagedata import Node
    moved, derived = [], []
    for s, nodes in enumerate(NODE_SETS):
        d["nodes_%d_values" % s] = np.array([v for v, _ in nodes])
        d["nodes_%d_colours" % s] = np.array([c for _, c in nodes], np.int64)
        me = types.SimpleNamespace(nodes=[Node(v, c) for v, c in nodes], from_=rs.WIDGET, buffer_slices={}, _type_projection=0)
        rs.Slice.UpdateColourTableBackgroundWidget(me, me.nodes)
        derived.append((me.window_width, me.window_level))
        for ww, wl in WWWL:
            me = types.SimpleNamespace(nodes=[Node(v, c) for v, c in nodes], from_=rs.WIDGET)
            rs.Slice._update_wwwl_widget_nodes(me, ww, wl)
            moved.append(np.array([n.value for n in me.nodes]))
    d["nodes_wwwl"] = np.array(WWWL)
    d["nodes_window_level"] = np.array(derived)
    for k, m in enumerate(moved):
        d["nodes_moved_%d" % k] = m

    # the colour dicts of GetSlices, captured from do_custom_colour's argument; get_aux_slice's indexing
    aux = np.arange(4 * 5 * 6, dtype=np.uint8).reshape(4, 5, 6)
    rs.converters.to_vtk = lambda m, *a, **k: m
    for label, show, shown, colours in (("watershed", "watershed", True, {}), ("default", "SELECT", False, {}),
                                       ("given", "SELECT", True, {"SELECT": {0: (0.0, 0.0, 0.0, 0.0), 7: (0.25, 0.5, 1.0, 0.75)}})):
        seen = {}
        me = types.SimpleNamespace(
            buffer_slices={"AXIAL": types.SimpleNamespace(index=-1, vtk_image=None, vtk_mask=None, mask=None)}, _type_projection=0,
            spacing=(1, 1, 1), opacity=0.4, to_show_aux=show, aux_matrices={show: aux}, aux_matrices_colours=colours,
            current_mask=types.SimpleNamespace(is_shown=shown), get_image_slice=lambda *a, **k: "image", do_ww_wl=lambda i: i,
            do_colour_image=lambda i: i, get_mask_slice=lambda *a: "mask", do_colour_mask=lambda m, o: m, do_blend=lambda a, b: (a, b))
        me.get_aux_slice = lambda name, o, n, me=me: rs.Slice.get_aux_slice(me, name, o, n)
        me.do_custom_colour = lambda img, table, seen=seen: seen.update(table=dict(table), image=np.array(img)) or "aux"
        rs.Slice.GetSlices(me, "AXIAL", 2, 1)
        keys = sorted(seen["table"])
        d["aux_%s_keys" % label] = np.array(keys, np.int64)
        d["aux_%s_rgba" % label] = np.array([seen["table"][k] for k in keys], np.float64)
        assert np.array_equal(seen["image"], aux[2])
    d["aux_matrix"] = aux
    for o in ("AXIAL", "CORONAL", "SAGITAL"):
        me = types.SimpleNamespace(aux_matrices={"m": aux})
        d["aux_slice_%s" % o] = rs.Slice.get_aux_slice(me, "m", o, 3)
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path), "bytes,", len(d), "arrays")


if __name__ == "__main__":
    main(os.path.join(HERE, "ref_slicedisplay.npz"))
