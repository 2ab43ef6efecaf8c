"""Golden vectors from the REFERENCE ITSELF: invesalius.data.mask3d_editor_state.Mask3DEditorState imported from
/root/reference and driven through scripts of tool events on small padded mask matrices.

    python3 tests/golden/make_golden_ref_mask3deditor.py

Set-up, as in the other make_golden_ref_*.py scripts:
* the module's GUI-side imports are satisfied by the stand-in finder of make_golden_ref_dowatershed.py;
* ``mask_cut`` / ``brush_mask_rs`` / ``polygon2mask_rs`` are bound to oracle/'s C restatement of invesalius_rs
  (oracle.mask_cut / brush_mask / polygon2mask); the brush gets a contiguous copy of the view it is given, written back;
* ``Slice``, ``Session`` and ``Publisher`` are recorders.  The Publisher also delivers: a message reaches the methods the
  state subscribed, and a viewer stand-in answers ``Send volume viewer size`` and ``Send volume viewer active camera`` at
  once, as the reference's viewer does.  With a viewport of height 0 the viewer stand-in does not answer the camera message:
  ReceiveVolumeViewerActiveCamera divides by the height;
* the current mask is a stand-in that holds the matrix; its ``modified`` and ``save_history`` are the reference's own
  functions (invesalius.data.mask.Mask) called on it, its history records ``new_node``;
* ``vtkCoordinate`` is a stand-in that applies this script's own world_to_display (VTK is not installed; PARITY UNPINNED), and
  the camera is a stand-in that returns this script's view and projection matrices.  Every (world point, display point) pair
  the stand-in computed is stored, so that a replay feeds the very same doubles to its rasteriser;
* ``PolygonSelectCanvas`` is a stand-in with ``_world_points``, ``complete``, ``insert_point`` and ``complete_polygon`` (at
  least three points): the state machine uses nothing else of it, and the real one pulls in the wx canvas.

Per script the .npz holds, as JSON: the spacing, the viewport, the clipping range, and the calls; after every call the whole
mask matrix, the whole ``mask_data``, ``has_cleared_for_crop`` and the messages sent.  What the port does differently is in
`notes`.  Nothing here is read at test time except the .npz it writes."""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

SHAPE = (6, 8, 10)  # the padded matrix: a (5, 7, 9) image
SPACING = (0.5, 0.75, 1.25)
SIZE = (40, 30)
CLIP = (2.0, 30.0)
NOTES = [
    "PolygonSelectCanvas is a stand-in (_world_points, complete, insert_point, complete_polygon): the real class imports the wx canvas",
    "vtkCoordinate / vtkCamera are numpy stand-ins of this script (VTK is not installed): PARITY UNPINNED",
    "the port calls CutMaskFromPolygons directly after publishing 'M3E cut mask from 3D'; it subscribes to nothing",
    "the port leaves viewer.canvas, Slice.discard_all_buffers and Mask._update_imagedata to its caller",
    "the port's get_filters returns display points; the rasters are made by one kernel in CutMaskFromPolygons",
    "with a viewport of height 0 the viewer stand-in does not answer 'Send volume viewer active camera' (the reference divides by it)",
    "save_history receives (original_mask_data, mask_data) as (array, p_array): kept in that order",
]

# ---- the camera: a parallel projection looking at the volume from the front, slightly off axis -------------------------------
FOCAL = np.array([2.0, -2.25, 2.5])
DIR = np.array([0.2, 1.0, -0.1]) / np.linalg.norm([0.2, 1.0, -0.1])
RIGHT = np.cross(DIR, [0.0, 0.0, 1.0]) / np.linalg.norm(np.cross(DIR, [0.0, 0.0, 1.0]))
UP = np.cross(RIGHT, DIR)
POSITION = FOCAL - 12.0 * DIR
SCALE = 4.0


def view_transform():
    v = np.eye(4)
    for i, axis in enumerate((RIGHT, UP, -DIR)):
        v[i, :3] = axis
        v[i, 3] = -float(axis @ POSITION)
    return v


def projection(aspect, nearz, farz):
    near, far = CLIP
    p = np.eye(4)
    p[0, 0] = 1.0 / (SCALE * aspect)
    p[1, 1] = 1.0 / SCALE
    p[2, 2] = -2.0 / (far - near)
    p[2, 3] = -(near + far) / (far - near)
    z = np.eye(4)
    z[2, 2] = (farz - nearz) / 2.0
    z[2, 3] = (farz + nearz) / 2.0
    return z @ p


def world_to_display(p, size):
    w, h = size
    v = projection(w / float(h), -1.0, 1.0) @ view_transform() @ np.array([p[0], p[1], p[2], 1.0])
    return (float((v[0] / v[3] + 1.0) * w / 2.0), float((v[1] / v[3] + 1.0) * h / 2.0))


def world_at(u, v):
    """a world point on the focal plane, u to the right and v up from the focal point"""
    return [float(x) for x in FOCAL + u * RIGHT + v * UP]


def scripts():
    P = lambda u, v: ["insert_point", [0.0, 0.0, world_at(u, v)]]  # noqa: E731  (the mouse position is not used by the state)
    tri = [P(-2.5, -2.0), P(2.0, -1.5), P(0.0, 2.5)]
    quad = [P(-3.5, 0.5), P(-1.0, 0.5), P(-1.0, 3.0), P(-3.5, 3.0)]
    sliver = [P(1.0, 1.0), P(3.5, 1.2), P(3.2, 3.0)]
    done = ["complete_current_polygon", []]
    setup = [["setup_state", []]]
    B = lambda x, y, z: ["brush_stroke", [[x, y, z]]]  # noqa: E731
    drag = [B(0.5 + 0.5 * k, -1.0 - 0.45 * k, 0.5 + 0.6 * k) for k in range(7)]
    return [
        {"name": "one polygon, exclude, depth 1.0 -> 0.5 -> 0.2", "steps": setup + tri + [done, ["SetDepthValue", [0.5]], ["SetDepthValue", [0.2]],
                                                                                         ["OnRestoreInitMask", []], ["cleanup_state", []]]},
        {"name": "one polygon, include", "steps": setup + [["SetEditMode", [0]]] + tri + [done, ["SetDepthValue", [0.5]]]},
        {"name": "three polygons, exclude, then a mode switch", "steps": setup + tri + [done] + quad + [done] + sliver + [done, ["SetEditMode", [0]],
                                                                                                                      ["SetEditMode", [1]]]},
        {"name": "three polygons, include, shallow first", "steps": setup + [["SetDepthValue", [0.45]], ["SetEditMode", [0]]] + tri + [done] + quad +
         [done] + sliver + [done, ["SetDepthValue", [1.0]]]},
        {"name": "an incomplete polygon in the list", "steps": setup + tri + [done] + quad[:2] + [["SetDepthValue", [0.9]], ["complete_current_polygon", []],
                                                                                                 quad[2], done, ["SetDepthValue", [0.8]]]},
        {"name": "ClearPolygons and OnMaskChanged", "steps": setup + tri + [done, ["ClearPolygons", []], ["SetDepthValue", [0.5]], ["host_edit", []],
                                                                            ["OnMaskChanged", [0]]] + quad + [done]},
        {"name": "brush: one dab and a drag of seven, erase", "preview": True,
         "steps": setup + [["SetToolMode", [1]], ["SetBrushSize", [3.0]], ["start_brush_stroke", []], B(2.0, -2.0, 2.5), ["end_brush_stroke", []],
                           ["start_brush_stroke", []]] + drag + [["end_brush_stroke", []]]},
        {"name": "brush: two include strokes in a row, then a third on the untouched result", "steps": setup + [
            ["SetEditMode", [0]], ["SetToolMode", [1]], ["SetBrushSize", [3.5]], ["start_brush_stroke", []], B(1.0, -1.5, 1.5), B(1.5, -2.0, 2.0),
            ["end_brush_stroke", []], ["start_brush_stroke", []], B(3.0, -3.5, 4.0), ["end_brush_stroke", []], ["host_restore", []],
            ["start_brush_stroke", []], B(2.0, -2.5, 3.0), ["end_brush_stroke", []]]},
        {"name": "a viewport of height 0", "steps": setup + tri + [["set_size", [40, 0]], done, B(2.0, -2.0, 2.5), ["set_size", [40, 30]],
                                                                   ["SetDepthValue", [0.6]]]},
        {"name": "no mask", "no_mask": True, "steps": setup + tri + [done, ["start_brush_stroke", []], B(2.0, -2.0, 2.5), ["end_brush_stroke", []],
                                                                      ["OnMaskChanged", [0]], ["ClearPolygons", []]]},
    ]


def main(path):
    from make_golden_ref_dowatershed import _Finder

    sys.meta_path.insert(0, _Finder())
    import pubsub.pub
    pubsub.pub.subscribe = lambda *a, **k: (None, True)
    sys.path.insert(0, "/root/reference")
    os.environ.setdefault("HOME", tempfile.mkdtemp())
    stand_in = types.ModuleType("invesalius.data.polygon_select")  # (the real module imports the wx canvas)
    stand_in.PolygonSelectCanvas = object
    sys.modules["invesalius.data.polygon_select"] = stand_in
    with contextlib.redirect_stdout(io.StringIO()):
        from invesalius.data import mask as ref_mask
        from invesalius.data import mask3d_editor_state as ref
    from oracle import oracle as orc
    orc.build()

    # -- invesalius_rs bound to the oracle
    def mask_cut(_image, sx, sy, sz, depth, filt, m, mv, out, edit_mode):
        orc.mask_cut(out, sx, sy, sz, depth, filt, m, mv, edit_mode)

    def brush_mask_rs(out, orig, spacing, center, radius, edit_mode):
        dense = np.ascontiguousarray(out)
        orc.brush_mask(dense, np.ascontiguousarray(orig) if orig is not None else None, spacing, center, radius, edit_mode)
        out[...] = dense

    ref.mask_cut, ref.brush_mask_rs, ref.polygon2mask_rs = mask_cut, brush_mask_rs, orc.polygon2mask
    ref.vtkarray_to_numpy = lambda m: np.array(m, np.float64)

    sent, subscribers, table = [], [], []
    world = {"state": None, "size": SIZE, "mask": None, "preview": False}

    class Publisher:
        @staticmethod
        def subscribe(listener, topic):
            subscribers.append((listener, topic))

        @staticmethod
        def sendMessage(topic, **kw):
            sent.append(topic)
            for listener, t in list(subscribers):
                if t == topic:
                    listener(**kw)
            st = world["state"]
            if topic == "Send volume viewer size":
                st.ReceiveVolumeViewerSize(world["size"])
            elif topic == "Send volume viewer active camera" and world["size"][1] != 0:
                st.ReceiveVolumeViewerActiveCamera(Camera())

    class Camera:
        def GetClippingRange(self):
            return CLIP

        def GetCompositeProjectionTransformMatrix(self, aspect, nearz, farz):
            return projection(aspect, nearz, farz) @ view_transform()

        def GetViewTransformMatrix(self):
            return view_transform()

    class Coordinate:
        def SetValue(self, p):
            self.p = tuple(float(v) for v in p)

        def GetComputedDoubleDisplayValue(self, renderer):
            d = world_to_display(self.p, world["size"])
            table.append(list(self.p) + list(d))
            return d

    class Polygon:
        def __init__(self):
            self._world_points, self.points, self.complete, self.visible = [], [], False, True

        def insert_point(self, display_point, world_point):
            self.points.append(display_point)
            self._world_points.append(world_point)

        def complete_polygon(self):
            if len(self.points) >= 3:
                self.complete = True

        def set_interactive(self, value):
            pass

    class Canvas:
        draw_list = []

    class Viewer:
        canvas, ren = Canvas(), object()

        def GetSize(self):
            return world["size"]

        def UpdateCanvas(self):
            pass

    class History:
        def __init__(self):
            self.nodes = []

        def new_node(self, index, orientation, array, p_array, clean):
            self.nodes.append((index, orientation, array.copy(), p_array.copy(), clean))

    class Mask:
        def __init__(self, matrix):
            self.matrix, self.was_edited, self.volume, self.history = matrix, False, None, History()
            self._modified_callbacks, self.modified_time = [], 0

        def modified(self, all_volume=False):
            ref_mask.Mask.modified(self, all_volume)

        def save_history(self, index, orientation, array, p_array, clean=False):
            ref_mask.Mask.save_history(self, index, orientation, array, p_array, clean)

    class TheSlice:
        spacing = SPACING

        @property
        def current_mask(self):
            return world["mask"]

        def discard_all_buffers(self):
            pass

    class TheSession:
        @property
        def mask_3d_preview(self):
            return world["preview"]

        def GetConfig(self, key, default=None):
            return False

    class _Mod:
        pass

    slc, ses = _Mod(), _Mod()
    slc.Slice, ses.Session = TheSlice, TheSession
    ref.slc, ref.ses, ref.Publisher, ref.vtkCoordinate, ref.PolygonSelectCanvas = slc, ses, Publisher, Coordinate, Polygon
    ref_mask.ses = ses

    data, out_scripts = {}, []
    rng = np.random.default_rng(20261)
    values = np.array([0, 1, 127, 128, 254, 255], np.uint8)
    for si, sc in enumerate(scripts()):
        del subscribers[:], table[:]
        Viewer.canvas.draw_list = []  # (ClearPolygons leaves a list on the instance)
        matrix = values[rng.integers(0, len(values), SHAPE)]
        matrix[1:, 1:, 1:][rng.random((SHAPE[0] - 1, SHAPE[1] - 1, SHAPE[2] - 1)) < 0.5] = 255  # mostly set: there is something to cut
        matrix[0, :, :] = matrix[:, 0, :] = matrix[:, :, 0] = 0
        start = matrix.copy()
        no_mask = bool(sc.get("no_mask"))
        world.update(size=SIZE, mask=None if no_mask else Mask(matrix), preview=bool(sc.get("preview")))
        st = world["state"] = ref.Mask3DEditorState(Viewer())
        steps = []
        for k, (call, args) in enumerate(sc["steps"]):
            del sent[:]
            if call == "set_size":
                world["size"] = tuple(args)
                steps.append({"call": call, "args": args})
                continue
            if call == "host_edit":  # another tool writes the mask between two uses of the editor
                matrix[2:4, 2:5, 3:8] = 255
                steps.append({"call": call, "args": []})
                continue
            if call == "host_restore":  # ... or puts back what the include stroke started from
                matrix[...] = start
                steps.append({"call": call, "args": []})
                continue
            with contextlib.redirect_stdout(io.StringIO()):
                getattr(st, call)(*args)
            step = {"call": call, "args": args, "sent": list(sent), "matrix": "", "mask_data": "", "has_cleared_for_crop": bool(st.has_cleared_for_crop)}
            if not no_mask:
                step["matrix"] = "s%d_%d_matrix" % (si, k)
                data[step["matrix"]] = matrix.copy()
            if st.mask_data is not None:
                step["mask_data"] = "s%d_%d_mask_data" % (si, k)
                data[step["mask_data"]] = np.array(st.mask_data, np.uint8)
            steps.append(step)
        entry = {"name": sc["name"], "spacing": list(SPACING), "size": list(SIZE), "clipping_range": list(CLIP), "matrix": "" if no_mask else "s%d_start" % si,
                 "m": "s%d_m" % si, "mv": "s%d_mv" % si, "mask_3d_preview": bool(sc.get("preview")), "display_table": [list(r) for r in table],
                 "history_nodes": 0 if no_mask else len(world["mask"].history.nodes), "steps": steps}
        if not no_mask:
            data[entry["matrix"]] = start
        aspect = SIZE[0] / float(SIZE[1])
        inv_y = np.diag([1.0, -1.0, 1.0, 1.0])
        data[entry["m"]] = st.world_to_screen if st.world_to_screen is not None else projection(aspect, *CLIP) @ view_transform() @ inv_y
        data[entry["mv"]] = st.world_to_camera_coordinates if st.world_to_camera_coordinates is not None else view_transform() @ inv_y
        out_scripts.append(entry)
    data["scripts"] = np.array(json.dumps(out_scripts))
    data["notes"] = np.array(NOTES)
    np.savez_compressed(path, **data)
    print(len(out_scripts), "scripts,", sum(len(s["steps"]) for s in out_scripts), "calls,", os.path.getsize(path), "bytes")
    for s in out_scripts:
        first = data[s["matrix"]] if s["matrix"] else None
        last = [st_["matrix"] for st_ in s["steps"] if st_.get("matrix")]
        print("  %-75s %s" % (s["name"], "" if first is None else "%d voxels changed" % int((data[last[-1]][1:, 1:, 1:] != first[1:, 1:, 1:]).sum())))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ref_mask3deditor.npz"))
