"""The deep-learning brain (MRI T1) and trachea (CT) segmentation on the GPU (segmentation/deep_learning/segment.py).

The reference runs the 3-D U-Net of model.py:9-113 with torch over overlapping 48^3 patches (segment_torch,
segment.py:162-191) and thresholds the averaged probabilities into a new mask (apply_segment_threshold, :465-490).  Here
the network is k_unet.hip (implicit-GEMM convolutions on the f32 matrix cores) behind the C ABI; the names below are the
reference's, at its signatures.  torch is never imported: `torch.save` files are read by a restricted unpickler that
knows the few globals a state dict needs and refuses every other one.

Numerics: normalisation, cuts, zero fill, crop, accumulation order and the division are numpy's, bit for bit; the
network's output differs from torch's float32 one by summation order only (DESIGN.md §7c gives the bound); the threshold
is the reference's float32 comparison, exactly.
"""
from __future__ import annotations

import ctypes
import io
import itertools
import os
import pickle
import zipfile
from collections import OrderedDict
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _lib as L

SIZE = 48
FEATURES = (8, 16, 32, 64, 128)
BN_EPS = 1e-5
DEFAULT_BATCH = 32  # patches per forward: ~12 MB of activations per 48^3 patch


@dataclass(frozen=True)
class SegmentPreset:
    """What BrainSegmentProcess / TracheaSegmentProcess fix (segment.py:505-541, 919-953) and the dialog's defaults."""
    name: str
    weights_file_name: str
    patch_size: int = SIZE
    overlap: int = 50
    threshold: float = 0.75            # deep_learning_seg_dialog.py:157
    mask_name_pattern: str = "brainseg_mri_t1"  # SegmentProcess.apply_segment_threshold, for both tools


PRESETS = {
    "brain": SegmentPreset("brain_mri_t1", "brain_mri_t1.pt"),
    "trachea": SegmentPreset("trachea_ct", "trachea_ct.pt"),
}
OVERLAPS = (0, 10, 25, 50)  # deep_learning_seg_dialog.py:86-87


# -- cuts ------------------------------------------------------------------------------------------------------------
def _axis_starts(n: int, patch_size: int, overlap_vox: int):
    s = [i for i in range(0, n, patch_size - overlap_vox) if i + patch_size <= n]
    if not s:
        s.append(0)
    elif s[-1] + patch_size < n:
        s.append(n - patch_size)
    return s


def _check_args(patch_size, overlap):
    if int(patch_size) != patch_size or patch_size < 16 or patch_size % 16:
        raise ValueError("patch_size must be a positive multiple of 16 (the network pools four times), got %r" % (patch_size,))
    if not 0 <= overlap < 100:
        raise ValueError("overlap must be in [0, 100), got %r" % (overlap,))


def patch_cuts(shape, patch_size: int, overlap: int):
    """gen_patches' cuts ((iz, ez), (iy, ey), (ix, ex)) in their order, without the patches."""
    _check_args(patch_size, overlap)
    ov = int(patch_size * overlap / 100)
    sz, sy, sx = (int(s) for s in shape)
    out = []
    for iz, iy, ix in itertools.product(_axis_starts(sz, patch_size, ov), _axis_starts(sy, patch_size, ov),
                                        _axis_starts(sx, patch_size, ov)):
        out.append(((iz, min(iz + patch_size, sz)), (iy, min(iy + patch_size, sy)), (ix, min(ix + patch_size, sx))))
    return out


def gen_patches(image: np.ndarray, patch_size: int, overlap: int):
    """segment.py:74-106: yields (completion, zero-filled float32 patch, cut) in itertools.product(z, y, x) order.
    The patch array is reused between iterations, as there."""
    cuts = patch_cuts(image.shape, patch_size, overlap)
    sub_image = np.empty((patch_size,) * 3, dtype="float32")
    for idx, ((iz, ez), (iy, ey), (ix, ex)) in enumerate(cuts):
        sub_image[:] = 0
        sub_image[: ez - iz, : ey - iy, : ex - ix] = image[iz:ez, iy:ey, ix:ex]
        yield (idx + 1.0) / len(cuts), sub_image, ((iz, ez), (iy, ey), (ix, ex))


def image_normalize_f32(image: np.ndarray) -> np.ndarray:
    """imagedata_utils.image_normalize(image, 0.0, 1.0, float32) as numpy 2 evaluates it on an int16 image (the reference
    of the device kernel; used by the tests)."""
    image = np.asarray(image)
    out = np.empty(image.shape, np.float32)
    imin, imax = image.min(), image.max()
    if imin == imax:
        out[:] = 0.0
        return out
    with np.errstate(over="ignore"):
        out[:] = (image - imin) * ((1.0 - 0.0) / (imax - imin)) + 0.0
    return out


# -- parameters ------------------------------------------------------------------------------------------------------
def _block_keys(prefix, name, cin, f):
    out = []
    for i, ci in ((1, cin), (2, f)):
        out += [("%s.%s_conv%d.weight" % (prefix, name, i), (f, ci, 5, 5, 5)), ("%s.%s_conv%d.bias" % (prefix, name, i), (f,))]
        for p in ("weight", "bias", "running_mean", "running_var"):
            out.append(("%s.%s_norm%d.%s" % (prefix, name, i, p), (f,)))
        out.append(("%s.%s_norm%d.num_batches_tracked" % (prefix, name, i), ()))
    return out


def param_spec():
    """[(key, shape)] of Unet3D().state_dict() in its order (model.py:9-113).  decoder3/2/1 reuse the layer prefix
    `dec4_` (model.py:39,44,49), so their keys read `decoder3.dec4_conv1.weight` and so on."""
    f = FEATURES
    spec = []
    cin = 1
    for i, (mod, name) in enumerate((("encoder1", "enc1"), ("encoder2", "enc2"), ("encoder3", "enc3"), ("encoder4", "enc4"),
                                     ("bottleneck", "bottleneck"))):
        spec += _block_keys(mod, name, cin, f[i])
        cin = f[i]
    for lvl in (4, 3, 2, 1):
        fo = f[lvl - 1]
        spec += [("upconv%d.weight" % lvl, (f[lvl], fo, 4, 4, 4)), ("upconv%d.bias" % lvl, (fo,))]
        spec += _block_keys("decoder%d" % lvl, "dec4", 2 * fo, fo)
    spec += [("conv.weight", (1, f[0], 1, 1, 1)), ("conv.bias", (1,))]
    return spec


def check_state_dict(sd) -> dict:
    """load_state_dict's strict check: missing and unexpected keys, and shapes, raise RuntimeError."""
    spec = param_spec()
    want = dict(spec)
    missing = [k for k, _ in spec if k not in sd]
    unexpected = [k for k in sd if k not in want]
    errs = []
    if missing:
        errs.append("Missing key(s) in state_dict: %s." % ", ".join('"%s"' % k for k in missing))
    if unexpected:
        errs.append("Unexpected key(s) in state_dict: %s." % ", ".join('"%s"' % k for k in unexpected))
    for k, shp in spec:
        if k in sd and tuple(np.shape(sd[k])) != shp:
            errs.append("size mismatch for %s: copying a param with shape %s, the model has %s." % (k, tuple(np.shape(sd[k])), shp))
    if errs:
        raise RuntimeError("Error(s) in loading state_dict for Unet3D:\n\t" + "\n\t".join(errs))
    return {k: np.asarray(sd[k]) for k, _ in spec}


def fold_params(sd) -> np.ndarray:
    """The float32 blob ivx_unet3d_load takes (include/ivx.h): BatchNorm folded into each conv in float64 --
    w * g / sqrt(v + eps), (b - m) * g / sqrt(v + eps) + beta -- rounded to float32 once."""
    sd = check_state_dict(sd)
    parts = []

    def conv_bn(prefix, name, i):
        w = sd["%s.%s_conv%d.weight" % (prefix, name, i)].astype(np.float64)
        b = sd["%s.%s_conv%d.bias" % (prefix, name, i)].astype(np.float64)
        g, beta, mu, var = (sd["%s.%s_norm%d.%s" % (prefix, name, i, p)].astype(np.float64)
                            for p in ("weight", "bias", "running_mean", "running_var"))
        s = g / np.sqrt(var + BN_EPS)
        parts.append((w * s[:, None, None, None, None]).astype(np.float32).ravel())
        parts.append(((b - mu) * s + beta).astype(np.float32))

    for mod, name in (("encoder1", "enc1"), ("encoder2", "enc2"), ("encoder3", "enc3"), ("encoder4", "enc4"),
                      ("bottleneck", "bottleneck")):
        conv_bn(mod, name, 1)
        conv_bn(mod, name, 2)
    for lvl in (4, 3, 2, 1):
        parts.append(sd["upconv%d.weight" % lvl].astype(np.float32).ravel())
        parts.append(sd["upconv%d.bias" % lvl].astype(np.float32))
        conv_bn("decoder%d" % lvl, "dec4", 1)
        conv_bn("decoder%d" % lvl, "dec4", 2)
    parts.append(sd["conv.weight"].astype(np.float32).ravel())
    parts.append(sd["conv.bias"].astype(np.float32))
    blob = np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)
    n = ctypes.c_int64(0)
    L.check(L.lib().ivx_unet3d_param_count(ctypes.byref(n)), "unet3d_param_count")
    assert blob.size == n.value, (blob.size, n.value)
    return blob


# -- weights files ---------------------------------------------------------------------------------------------------
_STORAGE_DTYPES = {
    "FloatStorage": np.float32, "DoubleStorage": np.float64, "HalfStorage": np.float16, "LongStorage": np.int64,
    "IntStorage": np.int32, "ShortStorage": np.int16, "CharStorage": np.int8, "ByteStorage": np.uint8,
    "BoolStorage": np.bool_, "BFloat16Storage": "bfloat16",
}


class _StorageType:
    def __init__(self, name):
        self.name = name


def _rebuild_tensor_v2(storage, storage_offset, size, stride, requires_grad=False, backward_hooks=None, metadata=None):
    size, stride = tuple(int(s) for s in size), tuple(int(s) for s in stride)
    if not size:
        return storage[storage_offset].copy()
    need = storage_offset + sum((s - 1) * st for s, st in zip(size, stride)) + 1 if all(size) else storage_offset
    if need > storage.size:
        raise ValueError("weights file: a tensor reaches past its storage")
    base = storage[storage_offset:]
    return np.lib.stride_tricks.as_strided(base, shape=size, strides=tuple(st * storage.itemsize for st in stride)).copy()


def _rebuild_parameter(data, requires_grad=False, backward_hooks=None):
    return data


class _RestrictedUnpickler(pickle.Unpickler):
    """Unpickles a torch.save state dict without torch: only OrderedDict, the two tensor rebuild functions and the storage
    type names resolve; any other global -- a pickle can name any callable -- raises pickle.UnpicklingError."""

    def __init__(self, f, zf, prefix):
        super().__init__(f)
        self._zf, self._prefix = zf, prefix
        self._storages = {}
        bo = prefix + "byteorder"
        self._order = "<"
        if bo in zf.namelist() and zf.read(bo).strip() == b"big":
            self._order = ">"

    def find_class(self, module, name):
        if (module, name) == ("collections", "OrderedDict"):
            return OrderedDict
        if (module, name) == ("torch._utils", "_rebuild_tensor_v2"):
            return _rebuild_tensor_v2
        if (module, name) == ("torch._utils", "_rebuild_parameter"):
            return _rebuild_parameter
        if module == "torch" and name in _STORAGE_DTYPES:
            return _StorageType(name)
        raise pickle.UnpicklingError("weights file names a forbidden global %s.%s" % (module, name))

    def persistent_load(self, pid):
        if not (isinstance(pid, tuple) and len(pid) == 5 and pid[0] == "storage" and isinstance(pid[1], _StorageType)):
            raise pickle.UnpicklingError("weights file: unsupported persistent id %r" % (pid,))
        _, st, key, _location, numel = pid
        if key not in self._storages:
            raw = self._zf.read("%sdata/%s" % (self._prefix, key))
            dt = _STORAGE_DTYPES[st.name]
            if dt == "bfloat16":
                u = np.frombuffer(raw, dtype=np.dtype(np.uint16).newbyteorder(self._order)).astype(np.uint32) << 16
                arr = u.view(np.float32)
            else:
                arr = np.frombuffer(raw, dtype=np.dtype(dt).newbyteorder(self._order)).astype(dt)
            if arr.size < int(numel):
                raise pickle.UnpicklingError("weights file: storage %s is truncated" % key)
            self._storages[key] = arr
        return self._storages[key]


def _read_torch_zip(path) -> dict:
    with zipfile.ZipFile(path) as zf:
        pkl = [n for n in zf.namelist() if n.endswith("/data.pkl") or n == "data.pkl"]
        if len(pkl) != 1:
            raise ValueError("%s: not a torch.save archive (no single data.pkl)" % path)
        prefix = pkl[0][: -len("data.pkl")]
        return _RestrictedUnpickler(io.BytesIO(zf.read(pkl[0])), zf, prefix).load()


def load_weights(weights) -> dict:
    """The state dict {key: ndarray} from a torch.save file (zip format, torch >= 1.6), an .npz, or a dict (either the
    state dict itself or a checkpoint holding it under "model_state_dict", as the reference's files do)."""
    if isinstance(weights, dict):
        d = weights
    else:
        path = Path(weights)
        if not path.exists():
            raise FileNotFoundError("Weights file not found")
        with open(path, "rb") as f:
            head = f.read(4)
        if head[:2] == b"PK":
            if str(path).endswith(".npz"):
                with np.load(path, allow_pickle=False) as z:
                    d = {k: z[k] for k in z.files}
            else:
                d = _read_torch_zip(path)
        elif head[:1] == b"\x80":
            raise ValueError("%s: legacy (pre-1.6, non-zip) torch.save format; re-save it with a newer torch "
                             "(torch.save(obj, f) writes the zip format)" % path)
        else:
            raise ValueError("%s: not a torch.save zip archive or .npz file" % path)
    if "model_state_dict" in d and isinstance(d["model_state_dict"], dict):
        d = d["model_state_dict"]
    return {k: np.asarray(v) for k, v in d.items()}


# -- the network on the device ---------------------------------------------------------------------------------------
class Unet3D:
    """The network resident in HBM (folded parameters); `weights` as for load_weights."""

    def __init__(self, weights):
        L.require_device()
        blob = fold_params(load_weights(weights))
        h = ctypes.c_void_p()
        L.check(L.lib().ivx_unet3d_load(L.ptr(blob), ctypes.c_int64(blob.size), ctypes.byref(h)), "unet3d_load")
        self.handle = h

    def workspace_bytes(self, patch_size: int, batch: int) -> int:
        nb = ctypes.c_size_t(0)
        L.check(L.lib().ivx_unet3d_workspace_bytes(self.handle, int(patch_size), int(batch), ctypes.byref(nb)),
                "unet3d_workspace_bytes")
        return nb.value

    def forward(self, patches: np.ndarray, batch: int = DEFAULT_BATCH) -> np.ndarray:
        """The raw network (model(x) of eval mode) on float32 patches (n, P, P, P) or (P, P, P) -> same shape."""
        from .device import DeviceBuffer

        x = np.ascontiguousarray(patches, dtype=np.float32)
        one = x.ndim == 3
        if one:
            x = x[None]
        if x.ndim != 4 or not (x.shape[1] == x.shape[2] == x.shape[3]):
            raise ValueError("patches must be (n, P, P, P)")
        P = x.shape[1]
        _check_args(P, 0)
        ws = DeviceBuffer(self.workspace_bytes(P, max(1, min(batch, x.shape[0]))))
        din, dout = DeviceBuffer(x.nbytes), DeviceBuffer(x.nbytes)
        try:
            din.upload(x)
            L.check(L.lib().ivx_dev_unet3d_forward(self.handle, din.ptr, ctypes.c_int64(x.shape[0]), int(P), dout.ptr,
                                                   ws.ptr, ctypes.c_size_t(ws.nbytes), None), "unet3d_forward")
            L.synchronize()
            out = dout.download(x.shape, np.float32)
        finally:
            for b in (ws, din, dout):
                b.close()
        return out[0] if one else out

    def close(self):
        if self.handle is not None and self.handle.value:
            L.lib().ivx_unet3d_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# -- one layer at a time (diagnostic: the tests compare each kernel with a float64 reference) ------------------------
def _run_layer(inputs, out_shape, call):
    """upload `inputs` (None stays None), run call(*device pointers, dst pointer), download float32 `out_shape`"""
    from .device import DeviceBuffer

    L.require_device()
    out_bytes = int(np.prod(out_shape)) * 4
    bufs = [None if a is None else DeviceBuffer(a.nbytes) for a in inputs] + [DeviceBuffer(out_bytes)]
    try:
        for b, a in zip(bufs, inputs):
            if b is not None:
                b.upload(a)
        bufs[-1].zero()
        call(*[None if b is None else b.ptr for b in bufs])
        L.synchronize()
        return bufs[-1].download(out_shape, np.float32)
    finally:
        for b in bufs:
            if b is not None:
                b.close()


def conv_layer(kind: int, x0: np.ndarray, w: np.ndarray, b: np.ndarray, x1: np.ndarray | None = None, relu: bool = False,
               tile=(0, 0)):
    """ivx_dev_unet3d_conv_layer: kind 0 = Conv3d(k 5, pad 2) with w (cout, cin, 5, 5, 5), kind 1 = ConvTranspose3d(k 4,
    s 2, p 1) with w (cin, cout, 4, 4, 4), on channels-last x0 (nb, S, S, S, c0) [and x1, torch.cat((x0, x1), channel)]
    -> (channels-last float32 output, (mt, nt) the kernel ran with).  `tile` forces that shape; (0, 0) is the forward's
    own choice."""
    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    x1 = None if x1 is None else np.ascontiguousarray(x1, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if x0.ndim != 5 or not (x0.shape[1] == x0.shape[2] == x0.shape[3]) or (x1 is not None and x1.shape[:4] != x0.shape[:4]):
        raise ValueError("activations must be channels-last (nb, S, S, S, C), both sources of one shape but for C")
    nb, S, c0 = x0.shape[0], x0.shape[1], x0.shape[4]
    c1 = 0 if x1 is None else x1.shape[4]
    cout = w.shape[0] if kind == 0 else w.shape[1]
    if w.shape != ((cout, c0 + c1, 5, 5, 5) if kind == 0 else (c0 + c1, cout, 4, 4, 4)) or b.shape != (cout,):
        raise ValueError("weights %s / bias %s do not fit kind %d with %d input channels" % (w.shape, b.shape, kind, c0 + c1))
    T = S if kind == 0 else 2 * S
    used = (ctypes.c_int(0), ctypes.c_int(0))

    def call(d0, d1, dst):
        L.check(L.lib().ivx_dev_unet3d_conv_layer(int(kind), d0, int(c0), d1, int(c1), L.ptr(w), L.ptr(b), int(cout), int(S),
                                                  int(nb), int(bool(relu)), int(tile[0]), int(tile[1]), dst,
                                                  ctypes.byref(used[0]), ctypes.byref(used[1]), None), "unet3d_conv_layer")

    out = _run_layer([x0, x1], (nb, T, T, T, cout), call)
    return out, (used[0].value, used[1].value)


def pool_layer(x: np.ndarray) -> np.ndarray:
    """ivx_dev_unet3d_pool_layer: MaxPool3d(2) on channels-last (nb, S, S, S, C) -> (nb, S/2, S/2, S/2, C)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 5 or not (x.shape[1] == x.shape[2] == x.shape[3]):
        raise ValueError("activations must be channels-last (nb, S, S, S, C)")
    nb, S, C = x.shape[0], x.shape[1], x.shape[4]

    def call(din, dst):
        L.check(L.lib().ivx_dev_unet3d_pool_layer(din, dst, int(S), int(C), int(nb), None), "unet3d_pool_layer")

    return _run_layer([x], (nb, S // 2, S // 2, S // 2, C), call)


def head_layer(x: np.ndarray, w: np.ndarray, b: float) -> np.ndarray:
    """ivx_dev_unet3d_head_layer: sigmoid(x @ w + b) on (nvox, 8) activations -> (nvox,) float32 probabilities"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] != 8 or np.size(w) != 8:
        raise ValueError("the head takes (nvox, 8) activations and 8 weights")
    w9 = np.ascontiguousarray(np.concatenate([np.ravel(w), [b]]), dtype=np.float32)

    def call(din, dst):
        L.check(L.lib().ivx_dev_unet3d_head_layer(din, L.ptr(w9), ctypes.c_int64(x.shape[0]), dst, None), "unet3d_head_layer")

    return _run_layer([x], (x.shape[0],), call)


def segment_unet3d(image: np.ndarray, weights, overlap: int = 50, patch_size: int = SIZE, apply_wwwl: bool = False,
                   window_width=255, window_level=127, probability_array: np.ndarray | None = None, comm_array=None,
                   batch: int = DEFAULT_BATCH) -> np.ndarray:
    """SegmentProcess._run_segmentation + segment_torch in one library call (ivx_segment_unet3d): the int16 image, with
    get_LUT_value(ww, wl) first if `apply_wwwl`, to the float32 probability map (added onto `probability_array`, zeros
    when not given, then divided by the cover count, as there)."""
    _check_args(patch_size, overlap)
    net = weights if isinstance(weights, Unet3D) else Unet3D(weights)
    image = np.asarray(image)
    if image.dtype != np.int16 or image.ndim != 3:
        raise TypeError("the segmentation takes the 3-D int16 image (Slice.matrix)")
    if any(s < 0 for s in image.strides):
        image = np.ascontiguousarray(image)
    if probability_array is None:
        probability_array = np.zeros(image.shape, np.float32)
    if probability_array.shape != image.shape or probability_array.dtype != np.float32:
        raise TypeError("probability_array must be float32 of the image's shape")
    dense = probability_array if probability_array.flags["C_CONTIGUOUS"] else np.ascontiguousarray(probability_array)
    prog = ctypes.c_float(0.0)
    L.check(L.lib().ivx_segment_unet3d(net.handle, L.ptr(image), L.i64(image.shape), L.i64(image.strides),
                                       int(bool(apply_wwwl)), ctypes.c_double(float(window_width)),
                                       ctypes.c_double(float(window_level)), int(patch_size), int(overlap), int(batch),
                                       L.ptr(dense), ctypes.byref(prog)), "segment_unet3d")
    if dense is not probability_array:
        probability_array[...] = dense
    if comm_array is not None:
        comm_array[0] = np.inf
    return probability_array


def segment_torch(image, weights_file, overlap, device_id, probability_array, comm_array, patch_size):
    """segment.py:162-191 at its signature, on HIP: `device_id` is accepted and ignored; `image` is the (LUT'd) int16
    image; the probabilities are added onto `probability_array` and divided by the cover count; comm_array[0] ends
    at inf."""
    weights_file = Path(weights_file)
    if not weights_file.exists():
        raise FileNotFoundError("Weights file not found")
    segment_unet3d(image, weights_file, overlap, patch_size, probability_array=probability_array, comm_array=comm_array)


def apply_segment_threshold(mask_matrix: np.ndarray, probability_array: np.ndarray, threshold: float) -> np.ndarray:
    """The mask write of SegmentProcess.apply_segment_threshold (segment.py:478-486): mask[1:, 1:, 1:] =
    (p >= float32(threshold)) * 255, then mask[:, 0, 0] = mask[0, :, 0] = mask[0, 0, :] = 2; the rest of the border
    planes keeps its bytes.  `mask_matrix` (uint8, shape + 1 per axis) is written in place and returned."""
    from .device import DeviceBuffer

    p = np.ascontiguousarray(probability_array, dtype=np.float32)
    if mask_matrix.dtype != np.uint8 or mask_matrix.shape != tuple(s + 1 for s in p.shape):
        raise TypeError("mask_matrix must be uint8 of the probability map's shape + 1 on each axis")
    L.require_device()
    m = np.ascontiguousarray(mask_matrix)
    dp, dm = DeviceBuffer(p.nbytes), DeviceBuffer(m.nbytes)
    try:
        dp.upload(p)
        dm.upload(m)
        L.check(L.lib().ivx_dev_segment_threshold(dp.ptr, L.i64(p.shape), ctypes.c_float(float(threshold)), dm.ptr,
                                                  L.i64([m.strides[0], m.strides[1], m.strides[2]]), 1, None),
                "segment_threshold")
        L.synchronize()
        out = dm.download(m.shape, np.uint8)
    finally:
        dp.close()
        dm.close()
    mask_matrix[...] = out
    return mask_matrix


def weights_path(preset: str, folder=None) -> Path:
    """Where the reference looks for a preset's weights file (segment.py:401-407) is the user's business here: nothing
    is downloaded; `folder` (default: the working directory) must hold the file the preset names."""
    return Path(folder or os.getcwd()) / PRESETS[preset].weights_file_name
