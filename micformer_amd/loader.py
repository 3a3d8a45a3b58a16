"""On-device head of the reference's input pipeline: raw CT / MR volumes (and the CT label volume) of a sample -> the float16
(2, D, H, W) image, the uint8 class map and `crop_indexes` that MMWHS_noCrop_Augment.__getitem__ produces on the CPU
(MMWHS.py:308-405, image_utils.py:48-55), on the HIP kernels of csrc/volume_loader.hip.

    from micformer_amd import data, loader
    ct, mr, lab = (torch.from_numpy(a).cuda(non_blocking=True) for a in (ct_arr, mr_arr, ct_label_arr))   # any (d, h, w) each
    image, label_map, crop = loader.load_batch([(ct, mr, lab), ...])        # fp16 [B,2,128,128,128], uint8 [B,128,128,128], int32 [B,3,2]
    x, y = data.prepare_raw_batch(image, label_map, params)                 # the device-side tail; y feeds MDiceLoss as it is

Geometric augmentation rides in the same pass (micformer_amd/affine.py has the rules; those calls run on csrc/volume_affine.hip):
    theta = affine.draw_affine(len(samples), generator=g, device="cuda")    # [B, 3, 4]: rotate / zoom / translate per sample
    image, label_map, crop = loader.load_batch(samples, affine=theta, padding_mode="border")
    theta.copy_(affine.draw_affine(len(samples), generator=g))              # a graph captured with out= reads the new draws
... and so does a smooth non-rigid deformation, composed with the map (micformer_amd/elastic.py; csrc/volume_elastic.hip):
    field = elastic.draw_elastic(len(samples), generator=g, device="cuda")  # [B, 3, 7, 7, 7]: a vector per control point
    image, label_map, crop = loader.load_batch(samples, displacement=field, field_interpolation="cubic", affine=theta)

What is computed, per sample (each array is resized independently from its own shape):
  * min-max normalisation of each image volume over the whole volume, (x - min) / (max - min), with one IEEE float32 divide per
    element.  A constant volume gives NaN everywhere, as the reference does.  NaN in the input is out of scope.
    `normalisation=` chooses "zscore" or "percentile" instead, for both channels or per channel (micformer_amd/normalise.py has
    the rules; those calls run on csrc/volume_normalise.hip, the default runs exactly as before).
  * trilinear resize (align_corners=False) of the normalised volumes to `size`, float16, channel 0 = CT, channel 1 = MR.
  * nearest resize of the CT label + lookup in `label_values` -> class map: 0 where the label is 0, k where it equals
    label_values[k - 1], 255 elsewhere.  (The reference's MR label planes are dropped by its `label[:8]` and are not computed.)
  * crop_indexes: per axis (max(0, min - 1), max + 1) of the voxels where resized CT + MR != 0; (0, 0) when the image is all zero
    (the reference raises there).

Two deliberate deviations from the reference: an int16 volume whose range exceeds 32767 is normalised with int32 arithmetic (the
reference's int16 `image - min` wraps), and the label is a uint8 class map with 255 for "no plane set" instead of 8 bool planes.

Nothing here synchronises with the host or runs an ATen compute op (allocation only); the launches go to the current stream and
can be captured by torch.cuda.graph when `out` is given.  The entry points are declared in include/micformer_loader.h; _lib.bind binds
them from this module's table (SIGNATURES below), which is apart from include/micformer_hip.h's.
"""
import ctypes

import torch

from . import _args, _lib, affine as _affine, elastic as _elastic, normalise

MMWHS_LABEL_VALUES = (205, 420, 500, 550, 600, 820, 850)          # MMWHS.py:289; class k = label_values[k - 1], class 0 = label 0
MAX_LABEL_VALUES = 254
DTYPE_I16, DTYPE_F32, DTYPE_I32 = 0, 1, 2
_IMAGE_DTYPES = {torch.int16: DTYPE_I16, torch.float32: DTYPE_F32}
_LABEL_DTYPES = {torch.int16: DTYPE_I16, torch.int32: DTYPE_I32}

# name -> argument signature (as _lib.SIGNATURES); the workspace query returns int64 (INT64_RETURNS), the other int
SIGNATURES = {
    "micf_volume_loader_workspace": "i",
    "micf_volume_loader": "piiiipiplpppp",
}
INT64_RETURNS = frozenset(("micf_volume_loader_workspace",))


class LoaderSample(ctypes.Structure):
    """struct micf_loader_sample (include/micformer_loader.h)."""
    _fields_ = [("ct", ctypes.c_void_p), ("mr", ctypes.c_void_p), ("label", ctypes.c_void_p),
                ("ct_shape", ctypes.c_int32 * 3), ("mr_shape", ctypes.c_int32 * 3), ("label_shape", ctypes.c_int32 * 3),
                ("ct_dtype", ctypes.c_int32), ("mr_dtype", ctypes.c_int32), ("label_dtype", ctypes.c_int32)]


lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="volume loader")


def _typed(t, what, dtypes):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise TypeError(f"{what} must be one of {sorted(str(d) for d in dtypes)}, got {t.dtype}")


def _volume(t, what, dtypes, device):
    if not t.is_cuda:
        raise ValueError(f"micformer_amd.loader runs on the GPU: {what} must be a CUDA (ROCm) tensor")
    if device is not None and t.device != device:
        raise ValueError(f"{what} is on {t.device}, the batch on {device}")
    if t.dim() != 3 or min(t.shape) < 1:
        raise ValueError(f"{what} must be a non-empty (d, h, w) volume, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return t.data_ptr(), tuple(t.shape), dtypes[t.dtype]


def _label_values(label_values):
    vals = _args.ints(label_values)
    if len(vals) > MAX_LABEL_VALUES:
        raise ValueError(f"at most {MAX_LABEL_VALUES} label values, got {len(vals)}")
    _args.distinct_nonzero(vals)
    _args.fit(vals, torch.int32)
    return _args.int32_array(vals), len(vals)


def load_batch(samples, size=(128, 128, 128), label_values=MMWHS_LABEL_VALUES, out=None, normalisation="minmax",
               percentiles=(1, 99), return_stats=False, displacement=None, field_interpolation="linear", affine=None,
               padding_mode="zeros"):
    """samples: sequence of (ct, mr, ct_label | None), every array an own-shaped (d, h, w) CUDA tensor (images int16 / float32,
    labels int16 / int32), labels present for all samples or for none.  out: optional preallocated (image, label_map,
    crop_indexes) to write into.  normalisation: "minmax" | "zscore" | "percentile", or a (ct, mr) pair of them; percentiles:
    (low, high) of the "percentile" mode.  return_stats=True appends the float64 [B, 2, 2] statistics of the normalisers.
    affine: optional float32 CUDA [B, 3, 4] (one map per sample) or [B, 2, 3, 4] (index 0 CT and label, index 1 MR), the
    F.affine_grid theta the resample reads on the device; padding_mode: "zeros" | "border", read only with `affine` or
    `displacement`.  displacement: optional float32 CUDA [B, 3, gd, gh, gw], a displacement field in normalised output coordinates
    on a control grid (micformer_amd/elastic.py), applied before `affine`; field_interpolation: "linear" | "cubic", read only with
    `displacement`.
    -> (image fp16 [B, 2, D, H, W], label_map uint8 [B, D, H, W] | None, crop_indexes int32 [B, 3, 2])[, stats]."""
    D, H, W = _args.triple(size, "size")
    vals, nvals = _label_values(label_values)
    ct_mode, mr_mode = normalise.modes(normalisation)
    p_low, p_high = normalise.percentile_pair(percentiles)
    if displacement is not None:
        _elastic.typed(displacement)
    if affine is not None:
        _affine.typed(affine)
    if displacement is not None and not isinstance(field_interpolation, str):
        _elastic.interpolation(field_interpolation)                 # (its TypeError before the first ValueError)
    if affine is not None or displacement is not None:
        pad = _affine.padding(padding_mode)
    if displacement is not None:
        interp = _elastic.interpolation(field_interpolation)
    samples = list(samples)
    if not samples:
        raise ValueError("load_batch needs at least one sample")
    B = len(samples)
    per_modality = _affine.maps(affine, B) if affine is not None else 0
    if displacement is not None:
        gd, gh, gw = _elastic.fields(displacement, B)
    items = (LoaderSample * B)()
    device, has_label = None, None
    for b, smp in enumerate(samples):
        if not isinstance(smp, (tuple, list)) or len(smp) != 3:
            raise ValueError(f"sample {b} must be a (ct, mr, ct_label | None) triple")
        ct, mr, lab = smp
        _typed(ct, f"sample {b}: ct", _IMAGE_DTYPES)                 # (types of the whole triple first: TypeError before ValueError)
        _typed(mr, f"sample {b}: mr", _IMAGE_DTYPES)
        if lab is not None:
            _typed(lab, f"sample {b}: ct_label", _LABEL_DTYPES)
        it = items[b]
        it.ct, shape, it.ct_dtype = _volume(ct, f"sample {b}: ct", _IMAGE_DTYPES, device)
        it.ct_shape[:] = shape
        device = ct.device
        it.mr, shape, it.mr_dtype = _volume(mr, f"sample {b}: mr", _IMAGE_DTYPES, device)
        it.mr_shape[:] = shape
        if has_label is None:
            has_label = lab is not None
        elif has_label != (lab is not None):
            raise ValueError("either every sample of a batch has a ct_label or none has")
        if lab is not None:
            it.label, shape, it.label_dtype = _volume(lab, f"sample {b}: ct_label", _LABEL_DTYPES, device)
            it.label_shape[:] = shape
    if out is None:
        image = torch.empty((B, 2, D, H, W), dtype=torch.float16, device=device)
        label_map = torch.empty((B, D, H, W), dtype=torch.uint8, device=device) if has_label else None
        crop = torch.empty((B, 3, 2), dtype=torch.int32, device=device)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 3:
            raise ValueError("out must be an (image, label_map | None, crop_indexes) triple")
        image = _args.out_tensor(out[0], "out image", (B, 2, D, H, W), torch.float16, device)
        if has_label != (out[1] is not None):
            raise ValueError("out label_map must be given exactly when the samples have labels")
        label_map = _args.out_tensor(out[1], "out label_map", (B, D, H, W), torch.uint8, device) if has_label else None
        crop = _args.out_tensor(out[2], "out crop_indexes", (B, 3, 2), torch.int32, device)
    if affine is not None and affine.device != device:
        raise ValueError(f"affine is on {affine.device}, the batch on {device}")
    if displacement is not None and displacement.device != device:
        raise ValueError(f"displacement is on {displacement.device}, the batch on {device}")
    warped = affine is not None or displacement is not None
    plain = not warped and (ct_mode, mr_mode) == (normalise.MINMAX, normalise.MINMAX) and not return_stats
    entry = "micf_volume_loader" + ("" if plain else "_norm" if not warped else "_affine" if displacement is None else "_elastic")
    stats = torch.empty((B, 2, 2), dtype=torch.float64, device=device) if return_stats else None
    nbytes = _lib.query_bytes(entry + "_workspace", B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    args = [ctypes.addressof(items), B, D, H, W, ctypes.addressof(vals), nvals]
    if not plain:
        args += [ct_mode, mr_mode, p_low, p_high]
    args += [ws.data_ptr(), nbytes, image.data_ptr(), None if label_map is None else label_map.data_ptr(), crop.data_ptr()]
    if not plain:
        args.append(None if stats is None else stats.data_ptr())
    if warped:
        args += [None if affine is None else affine.data_ptr(), per_modality, pad]
    if displacement is not None:
        args += [displacement.data_ptr(), gd, gh, gw, interp]
    _lib.call_on(device, entry, *args)
    return (image, label_map, crop, stats) if return_stats else (image, label_map, crop)


def load_pair(ct, mr, ct_label=None, size=(128, 128, 128), label_values=MMWHS_LABEL_VALUES, normalisation="minmax",
              percentiles=(1, 99), return_stats=False, displacement=None, field_interpolation="linear", affine=None,
              padding_mode="zeros"):
    """One sample: -> (image fp16 [2, D, H, W], label_map uint8 [D, H, W] | None, crop_indexes int32 [3, 2])[, stats float64
    [2, 2]].  affine: [3, 4] or [2, 3, 4]; displacement: [3, gd, gh, gw]."""
    if displacement is not None:
        _elastic.typed(displacement)
    if affine is not None:
        _affine.typed(affine)
    if displacement is not None and not isinstance(field_interpolation, str):
        _elastic.interpolation(field_interpolation)                  # (the keywords' TypeErrors before the first ValueError)
    if (affine is not None or displacement is not None) and not isinstance(padding_mode, str):
        _affine.padding(padding_mode)
    if displacement is not None:
        if displacement.dim() != 4:
            raise ValueError(f"displacement of load_pair must have shape [3, gd, gh, gw], got {list(displacement.shape)}")
        displacement = displacement.unsqueeze(0)                     # (a view: the kernel reads the caller's tensor)
    if affine is not None:
        if affine.dim() not in (2, 3):
            raise ValueError(f"affine of load_pair must have shape [3, 4] or [2, 3, 4], got {list(affine.shape)}")
        affine = affine.unsqueeze(0)                                 # (a view: the kernels read the caller's tensor)
    res = load_batch([(ct, mr, ct_label)], size=size, label_values=label_values, normalisation=normalisation,
                     percentiles=percentiles, return_stats=return_stats, displacement=displacement,
                     field_interpolation=field_interpolation, affine=affine, padding_mode=padding_mode)
    one = (res[0][0], None if res[1] is None else res[1][0], res[2][0])
    return one + (res[3][0],) if return_stats else one


__all__ = ["load_pair", "load_batch", "MMWHS_LABEL_VALUES", "SIGNATURES"]
