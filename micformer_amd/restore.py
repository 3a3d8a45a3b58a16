"""Predictions back to the geometry of the scan they came from: the inverse of `micformer_amd.loader`.  [B, K, D, H, W] float32
logits of the network grid -> per sample a label volume of its OWN shape (d, h, w) holding the dataset's label values, on the HIP
kernels of csrc/volume_restore.hip: trilinear upsample (align_corners=False) of the K class planes + argmax over K + class ->
label value in one fused pass.  The upsampled [K, d, h, w] tensor (3 GB at 8 x 363 x 512 x 512) is never written.

    from micformer_amd import loader, restore
    labels = restore.restore_labels(logits[0], ct.shape)                     # int16 (d, h, w): 0, 205, 420, ... 850
    labels = restore.restore_batch(logits, [ct.shape for ct in cts])         # a list, every sample with its own shape
    labels = restore.segment_pair(model, ct, mr)                             # raw CT / MR pair in, segmentation of the CT out

What is computed, per output voxel:
  * the coordinate rule of F.interpolate(mode="trilinear", align_corners=False) in float32, exactly (the rule the reference's loader
    applies in the other direction, MMWHS.py:332); only the order of the eight-product sum is this library's own.
  * probabilities=False interpolates the logits as they are; probabilities=True interpolates softmax(logits, 1), evaluated once per
    voxel of the LOW-resolution grid by a pre-pass (the two give different labels on the order of 1 % of the voxels).
  * argmax over K, the lowest class winning an exact tie; NaN logits are unspecified.
  * class 0 -> 0, class k -> label_values[k - 1] (`len(label_values) == K - 1`), stored as `dtype` (int16 / int32);
    label_values=None -> the uint8 class map itself.

Nothing here synchronises with the host or runs an ATen compute op (allocation only); the launches go to the current stream and
can be captured by torch.cuda.graph when `out` is given (with probabilities=True the capture then owns the softmax workspace, 64 MB
at 8 x 128^3, in the graph's memory pool).  The entry points are declared in include/micformer_restore.h; _lib.bind
binds them from this module's table (SIGNATURES below), which is apart from include/micformer_hip.h's.
"""
import ctypes

import torch

from . import _args, _lib
from ._args import MAX_CLASSES, MAX_EXTENT
from .loader import MMWHS_LABEL_VALUES

OUT_U8, OUT_I16, OUT_I32 = 0, 1, 2
LOGITS, PROBS = 0, 1
_OUT_DTYPES = {torch.int16: OUT_I16, torch.int32: OUT_I32}

# name -> argument signature (as _lib.SIGNATURES); the workspace query returns int64 (INT64_RETURNS), the other int
SIGNATURES = {
    "micf_volume_restore_workspace": "iiiiii",
    "micf_volume_restore": "piiiiipiipiplp",
}
INT64_RETURNS = frozenset(("micf_volume_restore_workspace",))


class RestoreSample(ctypes.Structure):
    """struct micf_restore_sample (include/micformer_restore.h)."""
    _fields_ = [("out", ctypes.c_void_p), ("out_shape", ctypes.c_int32 * 3)]


lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="volume restore")


def _label_values(label_values, K, dtype):
    vals = _args.ints(label_values)
    if len(vals) != K - 1:
        raise ValueError(f"{K} classes need {K - 1} label values (class 0 is always 0), got {len(vals)}")
    _args.fit(vals, dtype)
    return _args.int32_array(vals), len(vals)


def restore_batch(logits, shapes, label_values=MMWHS_LABEL_VALUES, probabilities=False, dtype=torch.int16, out=None):
    """logits: [B, K, D, H, W] float32 CUDA tensor, contiguous, 1 <= K <= 32.  shapes: one (d, h, w) per sample.  label_values: K - 1
    integers, or None for the uint8 class map.  out: optional list of B preallocated (d, h, w) tensors to write into.
    -> list of B label volumes (`dtype`, or uint8 with label_values=None)."""
    if not isinstance(logits, torch.Tensor):
        raise TypeError(f"logits must be a tensor, got {type(logits).__name__}")
    if logits.dtype != torch.float32:
        raise TypeError(f"logits must be torch.float32, got {logits.dtype}")
    if label_values is not None and dtype not in _OUT_DTYPES:
        raise TypeError(f"dtype must be torch.int16 or torch.int32, got {dtype}")
    if out is not None:
        if not isinstance(out, (tuple, list)) or not all(isinstance(t, torch.Tensor) for t in out):
            raise TypeError("out must be a list of tensors, one per sample")
    out_dtype = torch.uint8 if label_values is None else dtype
    # what does not depend on the device first (as loader.py checks `size` and `label_values`), then device and layout
    if logits.dim() != 5 or min(logits.shape) < 1:
        raise ValueError(f"logits must be a non-empty [B, K, D, H, W] tensor, got shape {tuple(logits.shape)}")
    B, K, D, H, W = logits.shape
    if K > MAX_CLASSES:
        raise ValueError(f"at most {MAX_CLASSES} classes, got {K}")
    if D * H * W > 512 ** 3:
        raise ValueError(f"at most 512^3 source voxels, got {D}x{H}x{W}")
    try:
        shapes = list(shapes)
    except TypeError:
        raise ValueError(f"shapes must be a sequence of (d, h, w), one per sample, got {shapes!r}") from None
    if len(shapes) != B:
        raise ValueError(f"{B} samples need {B} output shapes, got {len(shapes)}")
    shapes = [_args.triple(s, f"shape of sample {b}", MAX_EXTENT, 2 ** 31) for b, s in enumerate(shapes)]
    if label_values is None:
        vals, nvals = None, 0
    else:
        vals, nvals = _label_values(label_values, K, dtype)
    if not logits.is_cuda:
        raise ValueError("micformer_amd.restore runs on the GPU: logits must be a CUDA (ROCm) tensor")
    if not logits.is_contiguous():
        raise ValueError("logits must be contiguous")
    device = logits.device
    if out is None:
        out = [torch.empty(s, dtype=out_dtype, device=device) for s in shapes]
    else:
        if len(out) != B:
            raise ValueError(f"out must hold {B} tensors, got {len(out)}")
        out = [_args.out_tensor(t, f"out[{b}]", s, out_dtype, device) for b, (t, s) in enumerate(zip(out, shapes))]
    items = (RestoreSample * B)()
    for it, t, s in zip(items, out, shapes):
        it.out = t.data_ptr()
        it.out_shape[:] = s
    interpoland = PROBS if probabilities else LOGITS
    nbytes = _lib.query_bytes("micf_volume_restore_workspace", B, K, D, H, W, interpoland)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None
    _lib.call_on(device, "micf_volume_restore", logits.data_ptr(), B, K, D, H, W, ctypes.addressof(items),
                 OUT_U8 if label_values is None else _OUT_DTYPES[dtype], interpoland,
                 None if vals is None else ctypes.addressof(vals), nvals, None if ws is None else ws.data_ptr(), nbytes)
    return out


def restore_labels(logits, shape, label_values=MMWHS_LABEL_VALUES, probabilities=False, dtype=torch.int16, out=None):
    """One sample: logits [K, D, H, W] (or [1, K, D, H, W]) -> the (d, h, w) label volume."""
    if isinstance(logits, torch.Tensor) and logits.dim() == 4:
        logits = logits.unsqueeze(0)
    elif isinstance(logits, torch.Tensor) and (logits.dim() != 5 or logits.shape[0] != 1):
        raise ValueError(f"restore_labels takes one sample, [K, D, H, W] or [1, K, D, H, W], got shape {tuple(logits.shape)}")
    return restore_batch(logits, [shape], label_values=label_values, probabilities=probabilities, dtype=dtype,
                         out=None if out is None else [out])[0]


def segment_pair(model, ct, mr, size=(128, 128, 128), label_values=MMWHS_LABEL_VALUES, probabilities=False, keep_largest=False,
                 normalisation="minmax", percentiles=(1, 99), mirror_axes=()):
    """Raw CT / MR volumes of one sample (own-shaped (d, h, w) CUDA tensors, int16 / float32) -> the label volume of the CT's own
    shape: loader.load_pair -> data.prepare_raw_batch(image, None, None) (the validation transform) -> model under no_grad ->
    restore_labels at ct.shape.  keep_largest=True: the restored volume then goes through postprocess.keep_largest_components in
    place (of every class only its largest 26-connected component stays).  normalisation / percentiles: loader.load_pair's.
    mirror_axes: a subset of (0, 1, 2) = (D, H, W) for test-time mirroring; the logits are then mirror.mirrored_logits, the model's
    logits under each flip of these axes, flipped back and averaged (the input of a flip is a mirrored copy of the loaded image,
    bit for bit, and the validation transform runs on it inside the model as it does on the unflipped one)."""
    from . import data, loader, mirror
    mirrored = len(mirror.flip_codes(mirror_axes)) > 1
    image, _, _ = loader.load_pair(ct, mr, None, size=size, normalisation=normalisation, percentiles=percentiles)
    x, _ = data.prepare_raw_batch(image.unsqueeze(0), None, None)
    if mirrored:
        logits = mirror.mirrored_logits(model, x, mirror_axes)
    else:
        with torch.no_grad():
            logits = model(x)
    labels = restore_labels(logits.float().contiguous(), tuple(ct.shape), label_values=label_values, probabilities=probabilities)
    if keep_largest:
        from . import postprocess
        postprocess.keep_largest_components(labels, num_classes=int(logits.shape[1]), label_values=label_values, out=labels)
    return labels


__all__ = ["restore_batch", "restore_labels", "segment_pair", "MMWHS_LABEL_VALUES", "SIGNATURES"]
