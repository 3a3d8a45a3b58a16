"""Argument checks that loader, restore and postprocess perform identically.  Every one raises ValueError and touches no device;
the rules that belong to one front end (how many values, which dtypes) stay in that front end."""
import ctypes

import torch

MAX_CLASSES = 32          # MICF_RESTORE_MAX_CLASSES, MICF_COMPONENTS_MAX_CLASSES
MAX_EXTENT = 2048         # of one axis of a volume on the scan's grid


def ints(values, what="label_values"):
    try:
        return [int(v) for v in values]
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a sequence of integers, got {values!r}") from None


def int32_array(vals):
    """The host table a C entry point reads (one element at least, so that its address is never NULL)."""
    return (ctypes.c_int32 * max(len(vals), 1))(*vals)


def fit(vals, dtype, what="label_values"):
    info = torch.iinfo(dtype)
    if any(not info.min <= v <= info.max for v in vals):
        raise ValueError(f"{what} must fit in {dtype}")


def distinct_nonzero(vals, what="label_values"):
    if 0 in vals or len(set(vals)) != len(vals):
        raise ValueError(f"{what} must be distinct and non-zero (0 is always class 0), got {tuple(vals)}")


def triple(value, what, max_extent=None, max_voxels=None):
    """(d, h, w) as three integers >= 1, none above `max_extent`, their product below `max_voxels`."""
    rule = "three positive integers" if max_extent is None else f"three integers in 1..{max_extent}"
    if max_voxels is not None:
        rule += f" with fewer than {max_voxels} voxels"
    try:
        d, h, w = (int(s) for s in value)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be {rule}, got {value!r}") from None
    if (min(d, h, w) < 1 or (max_extent is not None and max(d, h, w) > max_extent)
            or (max_voxels is not None and d * h * w >= max_voxels)):
        raise ValueError(f"{what} must be {rule}, got {value!r}")
    return d, h, w


def out_tensor(t, what, shape, dtype, device):
    """A preallocated output: dtype, shape and device first, then contiguity."""
    shape = tuple(shape)
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or t.device != device:
        raise ValueError(f"{what} must be a {dtype} tensor of shape {shape} on {device}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return t
