"""Connected-component clean-up of a label volume, between `micformer_amd.restore` (the label volume on the scan's grid) and
`micformer_amd.metrics` (its score), on the HIP kernels of csrc/volume_components.hip: a 3-D union-find on the device, no host
round trip, a launch sequence that does not depend on the data.

    from micformer_amd import postprocess, restore
    labels = restore.segment_pair(model, ct, mr)                                  # int16 (d, h, w): 0, 205, 420, ... 850
    clean = postprocess.keep_largest_components(labels)                           # the largest component of every class
    clean = postprocess.remove_small_components(labels, min_size=64)
    comp, sizes = postprocess.connected_components(labels, return_sizes=True)     # int32 label and size per voxel

A volume is a (d, h, w) CUDA tensor, contiguous, either a uint8 class map (`label_values=None`: value k in 1..K-1 is class k,
K = `num_classes`) or an int16 / int32 label volume (value label_values[k - 1] is class k, K = len(label_values) + 1).  A list of
volumes, every one with its own shape, or a [B, d, h, w] tensor go through one call.  Value 0 is background; any other value that
names no class belongs to no component and is written through unchanged.

Rules (restated here, MONAI is not a dependency; include/micformer_components.h has them in full):
  * voxels are connected iff they hold the same class and are neighbours under `connectivity`: 6, 18 or 26 (the default, MONAI's
    full connectivity for 3-D); all classes in one pass (MONAI's independent=True).
  * a component's label is 1 + the smallest linear index (z * h + y) * w + x among its voxels (0 off-component): the order in
    which scipy.ndimage.label numbers them.  Its size is its voxel count.
  * keep-largest: per class of `classes` the component of the greatest size stays, the lowest label winning an exact tie
    (argmax of bincount, as MONAI / skimage); the class's other voxels become 0.  remove-small: size < min_size becomes 0.
Every result is an integer and bit-identical from run to run (integer atomics only).

Nothing here synchronises with the host or runs an ATen compute op (allocation only); the launches go to the current stream and
can be captured by torch.cuda.graph when `out` is given (the capture then owns the workspace, 8 bytes per voxel).  The entry
points are declared in include/micformer_components.h; _lib.bind binds them from this module's table (SIGNATURES below).
"""
import ctypes

import torch

from . import _args, _lib
from ._args import MAX_CLASSES, MAX_EXTENT
from .loader import MMWHS_LABEL_VALUES

MAX_VOXELS = 2 ** 31 - 1          # exclusive
IN_U8, IN_I16, IN_I32 = 0, 1, 2
KEEP_LARGEST, REMOVE_SMALL = 0, 1
_IN_DTYPES = {torch.uint8: IN_U8, torch.int16: IN_I16, torch.int32: IN_I32}

# name -> argument signature (as _lib.SIGNATURES); the workspace query returns int64 (INT64_RETURNS), the others int
SIGNATURES = {
    "micf_components_workspace": "pi",
    "micf_connected_components": "piiipiipplp",
    "micf_filter_components": "piiipiiliiplp",
}
INT64_RETURNS = frozenset(("micf_components_workspace",))


class ComponentSample(ctypes.Structure):
    """struct micf_component_sample (include/micformer_components.h)."""
    _fields_ = [("in_", ctypes.c_void_p), ("out", ctypes.c_void_p), ("shape", ctypes.c_int32 * 3)]


lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="connected components")


def _volumes(volume, what="volume"):
    """-> (list of (d, h, w) tensors, how to give the result back).  Checks what needs no device: dtype, shape and contiguity."""
    if isinstance(volume, torch.Tensor):
        if volume.dim() == 3:
            vols, pack = [volume], "one"
        elif volume.dim() == 4:
            vols, pack = list(volume.unbind(0)), "stack"
        else:
            raise ValueError(f"{what} must be (d, h, w), [B, d, h, w] or a list of (d, h, w) tensors, got shape {tuple(volume.shape)}")
    elif isinstance(volume, (list, tuple)) and volume and all(isinstance(t, torch.Tensor) for t in volume):
        vols, pack = list(volume), "list"
    else:
        raise TypeError(f"{what} must be a tensor or a non-empty list of tensors, got {type(volume).__name__}")
    if not vols:
        raise ValueError(f"{what} holds no sample")
    dtype = vols[0].dtype
    if dtype not in _IN_DTYPES:
        raise TypeError(f"{what} must be torch.uint8, torch.int16 or torch.int32, got {dtype}")
    for b, t in enumerate(vols):
        if t.dtype != dtype:
            raise TypeError(f"{what}[{b}] is {t.dtype}, the first sample {dtype}")
        if t.dim() != 3 or min(t.shape) < 1 or max(t.shape) > MAX_EXTENT or t.numel() >= MAX_VOXELS:
            raise ValueError(f"{what}[{b}] must be (d, h, w) with extents in 1..{MAX_EXTENT} and fewer than 2^31 - 1 voxels, "
                             f"got shape {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{what}[{b}] must be contiguous (w fastest), got strides {tuple(t.stride())}")
    return vols, pack


def _classes_of(dtype, num_classes, label_values):
    """-> (K, ctypes table or None, number of values)."""
    if dtype == torch.uint8:
        if num_classes is None and label_values is None:
            raise ValueError("a uint8 class map needs num_classes (or label_values, whose length + 1 it defaults to)")
        K = len(tuple(label_values)) + 1 if num_classes is None else num_classes
        vals = None
    else:
        if label_values is None:
            raise ValueError(f"an {dtype} label volume needs label_values (the value of every class but 0)")
        vals = _args.ints(label_values)
        K = len(vals) + 1 if num_classes is None else num_classes
    if isinstance(K, bool) or not isinstance(K, int) or not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"num_classes must be an integer in 2..{MAX_CLASSES}, got {K!r}")
    if vals is None:
        return K, None, 0
    if len(vals) != K - 1:
        raise ValueError(f"{K} classes need {K - 1} label values (class 0 is always 0), got {len(vals)}")
    _args.fit(vals, dtype)
    _args.distinct_nonzero(vals)
    return K, _args.int32_array(vals), len(vals)


def _connectivity(connectivity):
    if connectivity not in (6, 18, 26) or isinstance(connectivity, bool):
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    return int(connectivity)


def _class_mask(classes, K):
    if classes is None:
        return (1 << K) - 2
    try:
        ks = [k for k in classes]
    except TypeError:
        raise ValueError(f"classes must be a sequence of class indices in 1..{K - 1} or None, got {classes!r}") from None
    if not ks or any(isinstance(k, bool) or not isinstance(k, int) or not 1 <= k < K for k in ks):
        raise ValueError(f"classes must be a non-empty sequence of class indices in 1..{K - 1}, got {classes!r}")
    mask = 0
    for k in ks:
        mask |= 1 << k
    return mask


def _device_checks(vols, what="volume"):
    for b, t in enumerate(vols):
        if not t.is_cuda:
            raise ValueError(f"micformer_amd.postprocess runs on the GPU: {what}[{b}] must be a CUDA (ROCm) tensor")
        if t.device != vols[0].device:
            raise ValueError(f"{what}[{b}] is on {t.device}, the first sample on {vols[0].device}")


def _outputs(out, vols, pack, dtype, what="out"):
    """The list of output tensors for `vols` (allocated, or `out` checked) and the value to return."""
    device = vols[0].device
    if out is None:
        if pack == "stack":
            whole = torch.empty((len(vols),) + tuple(vols[0].shape), dtype=dtype, device=device)
            return list(whole.unbind(0)), whole
        outs = [torch.empty(tuple(t.shape), dtype=dtype, device=device) for t in vols]
        return outs, (outs[0] if pack == "one" else outs)
    if isinstance(out, torch.Tensor):
        if (pack == "one" and out.dim() == 3) or (pack == "list" and len(vols) == 1 and out.dim() == 3):
            outs = [out]
        elif pack == "stack" and out.dim() == 4 and out.shape[0] == len(vols):
            outs = list(out.unbind(0))
        else:
            raise ValueError(f"{what} must match the input: shape {tuple(out.shape)} does not")
        ret = out
    elif isinstance(out, (list, tuple)) and all(isinstance(t, torch.Tensor) for t in out):
        if pack != "list" or len(out) != len(vols):
            raise ValueError(f"{what} must match the input: a list of {len(vols)} tensors for a list of volumes")
        outs, ret = list(out), list(out)
    else:
        raise TypeError(f"{what} must be a tensor or a list of tensors")
    for b, (o, t) in enumerate(zip(outs, vols)):
        _args.out_tensor(o, f"{what}[{b}]", t.shape, dtype, device)
    return outs, ret


def _samples(vols, outs):
    items = (ComponentSample * len(vols))()
    for it, t, o in zip(items, vols, outs):
        it.in_ = t.data_ptr()
        it.out = o.data_ptr()
        it.shape[:] = tuple(t.shape)
    return items


def workspace_bytes(shapes):
    """Bytes of workspace of one call over volumes of these shapes (the library's own query)."""
    items = (ComponentSample * max(len(shapes), 1))()
    for it, s in zip(items, shapes):
        it.shape[:] = tuple(int(v) for v in s)
    return _lib.query_bytes("micf_components_workspace", ctypes.addressof(items), len(shapes))


def _workspace(items, B, device, workspace):
    nbytes = _lib.query_bytes("micf_components_workspace", ctypes.addressof(items), B)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
    elif workspace.dtype != torch.uint8 or workspace.device != device or workspace.numel() < nbytes or not workspace.is_contiguous():
        raise ValueError(f"workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {device}")
    return workspace, nbytes


def connected_components(volume, num_classes=None, label_values=MMWHS_LABEL_VALUES, connectivity=26, return_sizes=False, out=None,
                         workspace=None):
    """-> int32 labels shaped as `volume` (1 + the component's smallest linear index, 0 off-component); with return_sizes also the
    int32 size of every voxel's component (0 off-component).  `out`: preallocated labels, or (labels, sizes) with return_sizes."""
    vols, pack = _volumes(volume)
    K, vals, nvals = _classes_of(vols[0].dtype, num_classes, label_values)
    conn = _connectivity(connectivity)
    _device_checks(vols)
    out_l, out_s = (out if return_sizes and out is not None else (out, None))
    labels, ret_l = _outputs(out_l, vols, pack, torch.int32)
    sizes, ret_s = _outputs(out_s, vols, pack, torch.int32, "sizes") if return_sizes else (None, None)
    items = _samples(vols, labels)
    B = len(vols)
    device = vols[0].device
    ws, nbytes = _workspace(items, B, device, workspace)
    size_ptrs = (ctypes.c_void_p * B)(*[t.data_ptr() for t in sizes]) if return_sizes else None
    _lib.call_on(device, "micf_connected_components", ctypes.addressof(items), B, _IN_DTYPES[vols[0].dtype], K,
                 None if vals is None else ctypes.addressof(vals), nvals, conn,
                 None if size_ptrs is None else ctypes.addressof(size_ptrs), ws.data_ptr(), nbytes)
    return (ret_l, ret_s) if return_sizes else ret_l


def _filter(volume, mode, min_size, num_classes, label_values, connectivity, classes, out, workspace):
    vols, pack = _volumes(volume)
    K, vals, nvals = _classes_of(vols[0].dtype, num_classes, label_values)
    conn = _connectivity(connectivity)
    mask = _class_mask(classes, K)
    if isinstance(min_size, bool) or not isinstance(min_size, int) or not 1 <= min_size < 2 ** 31:
        raise ValueError(f"min_size must be an integer >= 1, got {min_size!r}")
    _device_checks(vols)
    outs, ret = _outputs(out, vols, pack, vols[0].dtype)
    items = _samples(vols, outs)
    B = len(vols)
    device = vols[0].device
    ws, nbytes = _workspace(items, B, device, workspace)
    _lib.call_on(device, "micf_filter_components", ctypes.addressof(items), B, _IN_DTYPES[vols[0].dtype], K,
                 None if vals is None else ctypes.addressof(vals), nvals, conn, mask, mode, min_size, ws.data_ptr(), nbytes)
    return ret


def keep_largest_components(volume, num_classes=None, label_values=MMWHS_LABEL_VALUES, connectivity=26, classes=None, out=None,
                            workspace=None):
    """The volume with, of every class of `classes` (class indices in 1..K-1, default all), only its largest component left; the
    lowest first voxel wins an exact tie.  `out` may be the input itself (in place)."""
    return _filter(volume, KEEP_LARGEST, 1, num_classes, label_values, connectivity, classes, out, workspace)


def remove_small_components(volume, min_size, num_classes=None, label_values=MMWHS_LABEL_VALUES, connectivity=26, classes=None,
                            out=None, workspace=None):
    """The volume without the components of fewer than `min_size` voxels (of the classes of `classes`, default all)."""
    return _filter(volume, REMOVE_SMALL, min_size, num_classes, label_values, connectivity, classes, out, workspace)


class KeepLargestConnectedComponent:
    """Callable under MONAI's name.  MONAI is not a dependency and its version is not pinned: the rules are restated, not
    imported -- independent=True (every class on its own, all in one pass), full connectivity (26) by default, the largest
    component by argmax of bincount (the lowest-numbered component wins an exact tie).  `applied_labels` are class indices."""

    def __init__(self, applied_labels=None, num_classes=None, label_values=MMWHS_LABEL_VALUES, connectivity=26):
        self.applied_labels, self.num_classes, self.label_values, self.connectivity = applied_labels, num_classes, label_values, connectivity

    def __call__(self, volume, out=None):
        return keep_largest_components(volume, self.num_classes, self.label_values, self.connectivity, self.applied_labels, out)


class RemoveSmallObjects:
    """Callable under MONAI's name (rules restated as for KeepLargestConnectedComponent: independent=True, full connectivity by
    default): components of fewer than `min_size` voxels become 0."""

    def __init__(self, min_size=64, connectivity=26, num_classes=None, label_values=MMWHS_LABEL_VALUES, applied_labels=None):
        self.min_size, self.connectivity, self.num_classes, self.label_values, self.applied_labels = (
            min_size, connectivity, num_classes, label_values, applied_labels)

    def __call__(self, volume, out=None):
        return remove_small_components(volume, self.min_size, self.num_classes, self.label_values, self.connectivity,
                                       self.applied_labels, out)


__all__ = ["connected_components", "keep_largest_components", "remove_small_components", "KeepLargestConnectedComponent",
           "RemoveSmallObjects", "workspace_bytes", "MMWHS_LABEL_VALUES", "SIGNATURES"]
