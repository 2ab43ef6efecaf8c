"""A numpy restatement of the mask edit history, for the tests: the `blocks64` snapshot format (encode, decode,
changed planes), the bookkeeping of EditionHistory over numpy-held nodes, and the driver that replays the scripts of
tests/golden/ref_history.npz against any history object.  Nothing here touches the GPU or the package."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_history.npz")


# ---- blocks64 -------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def layout(n):
    """B, W, offsets of literal[] and base[] in the header, header bytes"""
    B = cdiv(n, 64)
    W = cdiv(B, 64)
    off_lit = cdiv(B, 8) * 8
    off_base = off_lit + 8 * W
    return B, W, off_lit, off_base, off_base + 4 * W


def encode(x):
    """(header bytes, pool bytes, L) of the uint8 stream x"""
    x = np.ascontiguousarray(x, np.uint8).reshape(-1)
    n = x.size
    B, W, off_lit, off_base, hbytes = layout(n)
    padded = np.zeros(B * 64, np.uint8)
    padded[:n] = x
    blocks = padded.reshape(B, 64)
    value = blocks[:, 0].copy()
    valid = (np.arange(B * 64) < n).reshape(B, 64)
    lit = ((blocks != value[:, None]) & valid).any(axis=1)
    bits = np.zeros(W * 64, bool)
    bits[:B] = lit
    literal = (bits.reshape(W, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    counts = bits.reshape(W, 64).sum(axis=1)
    base = (np.cumsum(counts) - counts).astype(np.uint32)
    header = np.zeros(hbytes, np.uint8)
    header[:B] = value
    header[off_lit:off_base] = literal.view(np.uint8)
    header[off_base:] = base.view(np.uint8)
    pool = blocks[lit].reshape(-1).copy()  # (bytes past n are zeros already)
    return header, pool, int(lit.sum())


def decode(header, pool, n):
    B, W, off_lit, off_base, _ = layout(n)
    value = header[:B]
    literal = header[off_lit:off_base].view(np.uint64)
    base = header[off_base:].view(np.uint32)
    out = np.repeat(value, 64).reshape(B, 64).copy()
    for b in range(B):
        w, bit = b >> 6, b & 63
        word = int(literal[w])
        if (word >> bit) & 1:
            slot = int(base[w]) + bin(word & ((1 << bit) - 1)).count("1")
            out[b] = pool[64 * slot:64 * slot + 64]
    return out.reshape(-1)[:n].copy()


def changed_planes(old, new, plane_bytes):
    """flags: plane p holds a byte that differs between the two streams"""
    old, new = np.asarray(old).reshape(-1), np.asarray(new).reshape(-1)
    flags = np.zeros(cdiv(old.size, plane_bytes), np.uint8)
    flags[np.nonzero(old != new)[0] // plane_bytes] = 1
    return flags


# ---- the bookkeeping over numpy nodes ----------------------------------------------------------------------------------------------
def slice_view(matrix, orientation, index):
    if orientation == "AXIAL":
        return matrix[index + 1, 1:, 1:]
    if orientation == "CORONAL":
        return matrix[1:, index + 1, 1:]
    if orientation == "SAGITAL":
        return matrix[1:, 1:, index + 1]
    return matrix[:]


def flag_cell(orientation, index):
    return {"AXIAL": (index + 1, 0, 0), "CORONAL": (0, index + 1, 0), "SAGITAL": (0, 0, index + 1)}[orientation]


class NumpyNode:
    def __init__(self, index, orientation, array, clean):
        self.index, self.orientation, self.clean, self.array = index, orientation, clean, np.array(array, np.uint8)

    def commit(self, m):
        slice_view(m, self.orientation, self.index)[...] = self.array
        if self.clean and self.orientation != "VOLUME":
            m[flag_cell(self.orientation, self.index)] = 1


class NumpyHistory:
    """the rules, written as a state machine over (nodes, index): see DESIGN 7m"""

    def __init__(self, size=50, publish=None):
        self.history, self.index, self.cap, self.publish = [], -1, 2 * size, publish or (lambda *a, **k: None)
        self.publish("Enable undo", value=False)
        self.publish("Enable redo", value=False)

    def new_node(self, index, orientation, array, p_array, clean):
        for a in (p_array, array):
            if self.index == self.cap:
                del self.history[0]
                self.index -= 1
            del self.history[self.index + 1:]
            self.history.append(NumpyNode(index, orientation, a, clean))
            self.index += 1
            self.publish("Enable undo", value=True)
            self.publish("Enable redo", value=False)

    def _walk(self, mvolume, shown, step):
        """one undo (step -1) or redo (+1); returns True when the index moved"""
        h, at = self.history, self.index + step
        node = h[at]
        on_slice = lambda nd: bool(shown) and shown[nd.orientation] == nd.index  # noqa: E731
        if node.orientation != "VOLUME" and shown and not on_slice(node):
            self.publish(("Set scroll position", node.orientation), index=node.index)
            return False
        node.commit(mvolume)
        nxt = at + step
        if node.orientation != "VOLUME" and 0 <= nxt < len(h) and on_slice(h[nxt]):
            at = nxt
            h[at].commit(mvolume)
        self.index = at
        self.publish(("Set scroll position", h[at].orientation), index=h[at].index)
        return True

    def undo(self, mvolume, actual_slices=None):
        if not self.history:
            return
        if self.index > 0 and self._walk(mvolume, actual_slices, -1):
            self.publish("Enable redo", value=True)
        if self.index == 0:
            self.publish("Enable undo", value=False)

    def redo(self, mvolume, actual_slices=None):
        if not self.history:
            return
        if self.index < len(self.history) - 1 and self._walk(mvolume, actual_slices, +1):
            self.publish("Enable undo", value=True)
        if self.index == len(self.history) - 1:
            self.publish("Enable redo", value=False)

    def clear_history(self):
        self.history, self.index = [], -1
        self.publish("Enable undo", value=False)
        self.publish("Enable redo", value=False)

    def _config_undo_redo(self, visible):
        on = bool(self.history) and bool(visible)
        self.publish("Enable undo", value=on and self.index != 0)
        self.publish("Enable redo", value=on and (self.index == 0 or self.index != len(self.history) - 1))


# ---- the fixture and its driver ---------------------------------------------------------------------------------------------------
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(GOLDEN) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def script_names():
    return [str(n) for n in fixture()["names"]]


def replay(name, make_history, matrix, write=None, wrap=None):
    """Replays script `name` on `matrix` (filled with the script's initial state first) and compares matrix, index,
    len(history) and messages with the reference's after every operation.
    make_history(size, publish) -> the history under test; write(view, array): how the "tool" writes the matrix
    (default: numpy assignment); wrap(array, matrix, orientation) -> what new_node is handed for an array."""
    fx = fixture()
    script = json.loads(str(fx["script_" + name]))
    want_msgs = json.loads(str(fx["msg_" + name]))
    sent = []

    def publish(topic, **kw):
        sent.append([list(topic) if isinstance(topic, tuple) else topic, {k: (bool(v) if isinstance(v, bool) else int(v)) for k, v in kw.items()}])

    write = write or (lambda view, array: view.__setitem__(Ellipsis, array))
    wrap = wrap or (lambda array, m, orientation: array)
    write(matrix[:], fx["init_" + name])
    h = make_history(int(fx["size_" + name]), publish)
    assert sent == json.loads(str(fx["ctor_" + name])), "constructor messages"
    actual = {"AXIAL": 0, "CORONAL": 0, "SAGITAL": 0, "VOLUME": 0}
    for step, op in enumerate(script):
        del sent[:]
        if op[0] == "new":
            _, index, orientation, clean, k = op
            before, after = fx["parr_%s_%d" % (name, k)], fx["arr_%s_%d" % (name, k)]
            assert np.array_equal(slice_view(matrix, orientation, index), before), "step %d: the state before the edit" % step
            p = wrap(before, matrix, orientation)  # (a Snapshot of the matrix is taken before the tool writes)
            write(slice_view(matrix, orientation, index), after)
            h.new_node(index, orientation, wrap(after, matrix, orientation), p, clean)
        elif op[0] in ("undo", "redo"):
            getattr(h, op[0])(matrix, dict(actual) if op[1] else None)
        elif op[0] == "scroll":
            actual[op[1]] = op[2]
        elif op[0] == "clear":
            h.clear_history()
        elif op[0] == "config":
            h._config_undo_redo(op[1])
        for topic, kw in sent:
            if isinstance(topic, list) and topic[0] == "Set scroll position":
                actual[topic[1]] = kw["index"]
        where = "%s step %d %r" % (name, step, op)
        assert sent == want_msgs[step], "%s: messages %r, the reference sent %r" % (where, sent, want_msgs[step])
        assert h.index == fx["idx_" + name][step], "%s: index %d, the reference's %d" % (where, h.index, fx["idx_" + name][step])
        assert len(h.history) == fx["len_" + name][step], "%s: %d nodes, the reference has %d" % (where, len(h.history), fx["len_" + name][step])
        assert np.array_equal(matrix, fx["mat_" + name][step]), "%s: the matrix differs from the reference's" % where
    return h
