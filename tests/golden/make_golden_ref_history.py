"""Golden vectors from the REFERENCE ITSELF: invesalius.data.mask.EditionHistory imported from /root/reference and driven
through undo / redo scripts on small padded mask matrices.

    python3 tests/golden/make_golden_ref_history.py

The module's GUI-side imports are satisfied by the stand-in finder of make_golden_ref_dowatershed.py; EditionHistory is plain
python and touches none of them.  Its Publisher is replaced by a recorder, and a driver plays the GUI: a
``("Set scroll position", orientation)`` message moves the viewer, i.e. updates `actual_slices`.

A script is a list of operations (stored as JSON in the .npz, so the tests replay exactly what ran here):
    ["new", index, orientation, clean, k]   the tool's edit: array k is written into the matrix (the slice, or the whole
                                            matrix for VOLUME), then new_node(index, orientation, array k, the bytes
                                            that were there before, clean)
    ["undo", with_slices] / ["redo", with_slices]     with the viewer's actual_slices, or with None
    ["scroll", orientation, index]                    the user scrolls a viewer
    ["clear"] / ["config", visible]
After every operation the .npz holds the whole matrix, `index`, ``len(history)`` and the messages the operation sent.
Nothing here is read at test time except the .npz it writes.
"""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SHAPE = (6, 7, 8)  # the padded matrix: a (5, 6, 7) image


def slice_view(matrix, orientation, index):
    if orientation == "AXIAL":
        return matrix[index + 1, 1:, 1:]
    if orientation == "CORONAL":
        return matrix[1:, index + 1, 1:]
    if orientation == "SAGITAL":
        return matrix[1:, 1:, index + 1]
    return matrix[:]


def scripts():
    N = lambda i, o, c=False: ["new", i, o, c, None]  # noqa: E731  (the array numbers are filled in below)
    U, R, Un, Rn = ["undo", True], ["redo", True], ["undo", False], ["redo", False]
    s = {
        # every orientation, clean on and off; undone and redone with the viewer on the edited slice
        "orientations": [["scroll", "AXIAL", 2], N(2, "AXIAL"), ["scroll", "CORONAL", 3], N(3, "CORONAL", True), ["scroll", "SAGITAL", 1],
                         N(1, "SAGITAL"), N(0, "VOLUME"), ["scroll", "AXIAL", 4], N(4, "AXIAL", True), ["scroll", "SAGITAL", 5],
                         N(5, "SAGITAL", True), U, U, U, U, U, U, U, U, U, U, U, U, R, R, R, R, R, R, R, R, R, R, R, R],
        # the reference's callers that pass no actual_slices: every step is a single one
        "no_slices": [N(1, "AXIAL"), N(2, "CORONAL", True), N(0, "VOLUME"), Un, Un, Un, Un, Un, Un, Rn, Rn, Rn, Rn, Rn, Rn],
        # the viewer shows another slice: the first undo only scrolls, the second one is the real one (and so for redo)
        "scroll_only": [["scroll", "AXIAL", 0], N(0, "AXIAL"), ["scroll", "AXIAL", 3], N(3, "AXIAL"), ["scroll", "AXIAL", 0], U, U, U,
                        ["scroll", "AXIAL", 1], U, U, U, ["scroll", "AXIAL", 2], R, R, R, R, R, R],
        # the double step: two edits of the shown slice, a VOLUME node under a slice node, a slice node under a VOLUME node
        "double_step": [["scroll", "CORONAL", 2], N(2, "CORONAL"), N(2, "CORONAL", True), U, U, U, R, R, R, N(0, "VOLUME"), N(2, "CORONAL"),
                        U, U, U, U, R, R, R, R, N(0, "VOLUME"), U, U, U, R, R, R],
        # more nodes than a history of size 3 holds
        "overflow": [["scroll", "AXIAL", 1], N(1, "AXIAL"), N(0, "VOLUME"), N(1, "AXIAL", True), N(0, "VOLUME"), N(1, "AXIAL"), U, U, U, U, U, U,
                     U, U, R, R, R, R, R, R, R, R],
        # a new node after two undos drops the redo tail
        "truncation": [["scroll", "SAGITAL", 4], N(4, "SAGITAL"), N(0, "VOLUME"), N(4, "SAGITAL"), U, U, N(0, "VOLUME"), R, U, U, U, U, R, R, R,
                       R, R],
        # clear_history in the middle, the menu configuration, redo at the end, undo at index 0
        "clear": [["config", True], ["scroll", "AXIAL", 0], N(0, "AXIAL"), ["config", True], ["config", False], R, U, ["config", True], U, U, R, R, R,
                  N(0, "VOLUME"), ["clear"], ["config", True], N(0, "VOLUME"), U, U, U, R, R, R, ["clear"]],
    }
    sizes = {"overflow": 3}
    return s, sizes


def main(path):
    from make_golden_ref_dowatershed import _Finder

    sys.meta_path.insert(0, _Finder())
    import pubsub.pub
    pubsub.pub.subscribe = lambda *a, **k: (None, True)
    sys.path.insert(0, "/root/reference")
    os.environ.setdefault("HOME", tempfile.mkdtemp())
    with contextlib.redirect_stdout(io.StringIO()):
        from invesalius.data import mask as ref

    sent = []

    class Recorder:
        @staticmethod
        def sendMessage(topic, **kw):
            sent.append([list(topic) if isinstance(topic, tuple) else topic, {k: (bool(v) if isinstance(v, (bool, np.bool_)) else int(v)) for k, v in kw.items()}])

    ref.Publisher = Recorder
    data, names = {}, []
    all_scripts, sizes = scripts()
    rng = np.random.default_rng(20260)
    values = np.array([0, 1, 2, 253, 254, 255], np.uint8)
    for name, script in all_scripts.items():
        matrix = values[rng.integers(0, 6, SHAPE)]
        matrix[0, :, :] = matrix[:, 0, :] = matrix[:, :, 0] = 0  # the flag planes start clean
        data["init_" + name] = matrix.copy()
        actual = {"AXIAL": 0, "CORONAL": 0, "SAGITAL": 0, "VOLUME": 0}
        out = io.StringIO()
        with contextlib.redirect_stdout(out):  # (the reference prints a trace of every step)
            del sent[:]
            h = ref.EditionHistory(**({"size": sizes[name]} if name in sizes else {}))
            ctor = list(sent)
            mats, idx, lens, msgs, k = [], [], [], [], 0
            for op in script:
                del sent[:]
                if op[0] == "new":
                    _, index, orientation, clean, _k = op
                    view = slice_view(matrix, orientation, index)
                    before = view.copy()
                    after = values[rng.integers(0, 6, view.shape)]
                    if orientation == "VOLUME":  # a whole-matrix tool changes a few planes, not all of them
                        after = before.copy()
                        after[2:4] = values[rng.integers(0, 6, after[2:4].shape)]
                    op[4] = k
                    data["arr_%s_%d" % (name, k)], data["parr_%s_%d" % (name, k)] = after.copy(), before
                    k += 1
                    view[...] = after
                    h.new_node(index, orientation, after, before, clean)
                elif op[0] in ("undo", "redo"):
                    getattr(h, op[0])(matrix, dict(actual) if op[1] else None)
                elif op[0] == "scroll":
                    actual[op[1]] = op[2]
                elif op[0] == "clear":
                    h.clear_history()
                elif op[0] == "config":
                    h._config_undo_redo(op[1])
                for topic, kw in sent:  # the GUI's side of the scroll message
                    if isinstance(topic, list) and topic[0] == "Set scroll position":
                        actual[topic[1]] = kw["index"]
                mats.append(matrix.copy())
                idx.append(h.index)
                lens.append(len(h.history))
                msgs.append(list(sent))
        data["script_" + name] = np.array(json.dumps(script))
        data["size_" + name] = np.array(sizes.get(name, 50))
        data["ctor_" + name] = np.array(json.dumps(ctor))
        data["mat_" + name] = np.array(mats, np.uint8)
        data["idx_" + name] = np.array(idx, np.int64)
        data["len_" + name] = np.array(lens, np.int64)
        data["msg_" + name] = np.array(json.dumps(msgs))
        names.append(name)
        del h
    # the one stated deviation: what the reference does with an empty history
    notes = []
    with contextlib.redirect_stdout(io.StringIO()):
        for what in ("undo", "redo"):
            h = ref.EditionHistory()
            del sent[:]
            try:
                getattr(h, what)(np.zeros(SHAPE, np.uint8), None)
                notes.append("%s on an empty history: returned, messages %s" % (what, json.dumps(sent)))
            except IndexError as e:
                notes.append("%s on an empty history: IndexError(%s) in the trace print, after the messages %s; "
                             "history.EditionHistory does nothing instead" % (what, e, json.dumps(sent)))
    data["notes"] = np.array(notes)
    data["names"] = np.array(names)
    np.savez_compressed(path, **data)
    print(len(names), "scripts:", ", ".join("%s (%d calls)" % (n, len(data["idx_" + n])) for n in names))
    print("\n".join(notes))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ref_history.npz"))
