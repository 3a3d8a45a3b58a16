"""On-device surface distances in physical units: percentile Hausdorff distance, average (symmetric) surface distance and
surface Dice at a tolerance, on a grid with a voxel spacing per sample (MONAI's SurfaceDistanceMetric / SurfaceDiceMetric /
HausdorffDistanceMetric semantics with a `spacing`), on the HIP kernels of csrc/surface_distance.hip.

    from micformer_amd.surface import surface_distances
    r = surface_distances(labels, gt_labels, spacing=(1.6, 0.43, 0.43), percentiles=(95,), thresholds=[1.0] * 7)
    r.hd, r.assd, r.nsd                 # float32 [B, K', 1], [B, K'], [B, K'] on the device, in the spacing's unit

Inputs, both in the same form:
  * uint8 class maps [B, D, H, W] (`num_classes` required), or one-hot planes [B, K, D, H, W], as micformer_amd.metrics takes them;
  * int16 / int32 label volumes [B, D, H, W] (or one (D, H, W) volume): value label_values[k - 1] is class k, every other value is
    class 0, K = len(label_values) + 1 -- what restore_batch returns and what a raw ground-truth label file holds.
Edge sets are those of metrics.hausdorff_distance; at spacing (1, 1, 1) `hd` equals it bit for bit.  Nothing here synchronises
with the host, and every result is bit-identical from run to run.  The entry points are declared in
include/micformer_surface.h; _lib.bind binds them from this module's table (SIGNATURES below).  Rules: DESIGN.md "Surface
distances in millimetres".
"""
import ctypes
import math
from collections import namedtuple

import torch

from . import _args, _lib
from .loader import MMWHS_LABEL_VALUES
from .metrics import FORM_LABEL, FORM_ONEHOT, _first_class

FORM_VALUES_I16, FORM_VALUES_I32 = 2, 3
MAX_PERCENTILES = 4           # MICF_SURFACE_MAX_PERCENTILES
_VALUE_FORMS = {torch.int16: FORM_VALUES_I16, torch.int32: FORM_VALUES_I32}

# name -> argument signature (as _lib.SIGNATURES); the workspace query returns int64 (INT64_RETURNS), the other int
SIGNATURES = {
    "micf_surface_distance_workspace": "iiiii",
    "micf_surface_distance": "ppiiiiiiipippipplpp",
}
INT64_RETURNS = frozenset(("micf_surface_distance_workspace",))

lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="surface distances")

SurfaceDistances = namedtuple("SurfaceDistances", "hd hd_directed asd assd nsd")
SurfaceDistances.__doc__ = """hd, hd_directed: [B, K', P] (max of both directions / pred -> gt only, per requested percentile);
asd: [B, K', 2] (pred -> gt, gt -> pred); assd, nsd: [B, K'] (nsd is None without thresholds).  float32 views of one device buffer."""


def _double_array(vals):
    return (ctypes.c_double * max(len(vals), 1))(*vals)


def _forms(y_pred, y, num_classes, label_values):
    """-> (form, B, K, D, H, W, vals) of the three input forms; touches no device."""
    if not isinstance(y_pred, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise TypeError("y_pred and y must be tensors")
    if y_pred.shape != y.shape:
        raise ValueError(f"y_pred and y must have the same shape, got {tuple(y_pred.shape)} and {tuple(y.shape)}")
    if y_pred.dim() == 5:
        B, K, D, H, W = y_pred.shape
        if num_classes is not None and int(num_classes) != K:
            raise ValueError(f"num_classes={num_classes} does not match the {K} planes")
        return FORM_ONEHOT, B, K, D, H, W, None
    if y_pred.dim() != 4:
        raise ValueError("expected a class map or label volume [B, D, H, W] or one-hot planes [B, K, D, H, W], "
                         f"got {y_pred.dim()}-D")
    if y_pred.dtype != y.dtype or y_pred.dtype not in (torch.uint8, torch.int16, torch.int32):
        raise TypeError("a 4-D input is a uint8 class map or an int16 / int32 label volume, the same for y_pred and y; "
                        f"got {y_pred.dtype} and {y.dtype}")
    B, D, H, W = y_pred.shape
    if y_pred.dtype == torch.uint8:
        if num_classes is None:
            raise ValueError("class-map inputs need num_classes")
        return FORM_LABEL, B, int(num_classes), D, H, W, None
    if label_values is None:
        raise ValueError(f"an {y_pred.dtype} label volume needs label_values (the value of every class but 0)")
    vals = _args.ints(label_values)
    _args.distinct_nonzero(vals)
    _args.fit(vals, y_pred.dtype)
    K = len(vals) + 1
    if num_classes is not None and int(num_classes) != K:
        raise ValueError(f"num_classes={num_classes} does not match the {len(vals)} label values")
    return _VALUE_FORMS[y_pred.dtype], B, K, D, H, W, vals


def _spacing(spacing, B):
    """One (s_z, s_y, s_x) or one per sample (host data) -> 3 B floats, each > 0 and finite."""
    if spacing is None:
        return [1.0] * (3 * B)
    what = f"spacing must be (s_z, s_y, s_x) or one such triple for each of the {B} samples, as host numbers"
    if isinstance(spacing, torch.Tensor) and spacing.is_cuda:
        raise ValueError(f"{what}; got a device tensor")
    try:
        t = torch.as_tensor(spacing, dtype=torch.float64)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what}; got {spacing!r}") from None
    if tuple(t.shape) == (3,):
        t = t.expand(B, 3)
    if tuple(t.shape) != (B, 3):
        raise ValueError(f"{what}; got shape {tuple(t.shape)}")
    rows = [float(v) for v in t.reshape(-1)]
    if any(not (v > 0.0 and math.isfinite(v)) for v in rows):
        raise ValueError(f"every spacing must be positive and finite, got {spacing!r}")
    return rows


def _percentiles(percentiles):
    try:
        pct = [0.0 if not p else float(p) for p in percentiles]
    except TypeError:
        raise ValueError(f"percentiles must be a sequence of numbers (None = the maximum), got {percentiles!r}") from None
    if not 1 <= len(pct) <= MAX_PERCENTILES:
        raise ValueError(f"between 1 and {MAX_PERCENTILES} percentiles per call, got {len(pct)}")
    if any(not 0.0 <= p <= 100.0 for p in pct):
        raise ValueError(f"percentile should be a value between 0 and 100, got {tuple(percentiles)}")
    return pct


def _thresholds(thresholds, Kc):
    if thresholds is None:
        return None
    try:
        tau = [float(t) for t in thresholds]
    except (TypeError, ValueError):
        raise ValueError(f"class_thresholds must be a sequence of numbers, got {thresholds!r}") from None
    if len(tau) != Kc:
        raise ValueError(f"{Kc} scored classes need {Kc} class_thresholds, got {len(tau)}")
    if any(not t >= 0.0 for t in tau):
        raise ValueError(f"every class threshold must be >= 0, got {tuple(thresholds)}")
    return tau


def workspace_bytes(shape, K):
    """Bytes of workspace for inputs of `shape` ([B, D, H, W] or [B, K, D, H, W]) and K classes."""
    B, (D, H, W) = int(shape[0]), (int(s) for s in shape[-3:])
    return _lib.query_bytes("micf_surface_distance_workspace", B, int(K), D, H, W)


def surface_distances(y_pred, y, num_classes=None, label_values=MMWHS_LABEL_VALUES, include_background=False, spacing=None,
                      percentiles=(95,), thresholds=None, workspace=None):
    """Every surface distance of one (y_pred, y) pair in one call -> SurfaceDistances.  spacing: (s_z, s_y, s_x) or one per
    sample, default (1, 1, 1).  percentiles: up to 4, None / 0 = the maximum.  thresholds: one tolerance per scored class in the
    spacing's unit, or None for no surface Dice.  workspace: an optional uint8 CUDA tensor of workspace_bytes() bytes."""
    if isinstance(y_pred, torch.Tensor) and isinstance(y, torch.Tensor) and y_pred.dim() == 3 and y.dim() == 3:
        y_pred, y = y_pred.unsqueeze(0), y.unsqueeze(0)                     # one (D, H, W) volume, as restore_labels returns it
    # what does not depend on the device first, then device and layout
    form, B, K, D, H, W, vals = _forms(y_pred, y, num_classes, label_values)
    first = _first_class(include_background, K)
    Kc = K - first
    sp, pct, tau = _spacing(spacing, B), _percentiles(percentiles), _thresholds(thresholds, Kc)
    P = len(pct)
    if not (y_pred.is_cuda and y.is_cuda):
        raise ValueError("micformer_amd.surface runs on the GPU: y_pred and y must be CUDA (ROCm) tensors")
    if form == FORM_ONEHOT:
        pred, gt = y_pred.float().contiguous(), y.float().contiguous()
    else:
        pred, gt = y_pred.contiguous(), y.contiguous()
    nbytes = _lib.query_bytes("micf_surface_distance_workspace", B, K, D, H, W)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    else:
        if (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != pred.device
                or not workspace.is_contiguous() or workspace.numel() < nbytes):
            raise ValueError(f"workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {pred.device}")
    out = torch.empty(B * Kc * (2 * P + 4), dtype=torch.float32, device=pred.device)
    c_vals = None if vals is None else _args.int32_array(vals)
    c_sp, c_pct = _double_array(sp), _double_array(pct)
    c_tau = None if tau is None else _double_array(tau)
    _lib.call_on(pred.device, "micf_surface_distance", pred.data_ptr(), gt.data_ptr(), form, B, K, D, H, W, first,
                 None if c_vals is None else ctypes.addressof(c_vals), 0 if vals is None else len(vals), ctypes.addressof(c_sp),
                 ctypes.addressof(c_pct), P, None if c_tau is None else ctypes.addressof(c_tau), workspace.data_ptr(),
                 workspace.numel(), out.data_ptr())
    n = B * Kc
    hd = out[:n * P].view(B, Kc, P)
    hdd = out[n * P:2 * n * P].view(B, Kc, P)
    asd = out[2 * n * P:2 * n * P + 2 * n].view(B, Kc, 2)
    assd = out[2 * n * P + 2 * n:2 * n * P + 3 * n].view(B, Kc)
    nsd = out[2 * n * P + 3 * n:].view(B, Kc) if tau is not None else None
    return SurfaceDistances(hd, hdd, asd, assd, nsd)


def _euclidean(distance_metric):
    if distance_metric != "euclidean":
        raise ValueError(f"distance_metric {distance_metric!r} is not implemented (only 'euclidean')")


def hausdorff_distance_mm(y_pred, y, num_classes=None, label_values=MMWHS_LABEL_VALUES, include_background=False, spacing=None,
                          percentile=None, directed=False):
    """metrics.hausdorff_distance with a spacing: float32 [B, K'] in the spacing's unit."""
    r = surface_distances(y_pred, y, num_classes, label_values, include_background, spacing, (percentile,))
    return (r.hd_directed if directed else r.hd)[..., 0]


def average_surface_distance(y_pred, y, num_classes=None, label_values=MMWHS_LABEL_VALUES, include_background=False,
                             spacing=None, symmetric=False):
    """MONAI's compute_average_surface_distance: the mean distance pred -> gt, or with symmetric=True the mean over both
    directions' distances together.  float32 [B, K']."""
    r = surface_distances(y_pred, y, num_classes, label_values, include_background, spacing)
    return r.assd if symmetric else r.asd[..., 0]


def surface_dice(y_pred, y, class_thresholds, num_classes=None, label_values=MMWHS_LABEL_VALUES, include_background=False,
                 spacing=None):
    """MONAI's compute_surface_dice (use_subvoxels=False): the share of both surfaces within the class's tolerance of the other
    surface.  float32 [B, K']."""
    return surface_distances(y_pred, y, num_classes, label_values, include_background, spacing, thresholds=class_thresholds).nsd


class SurfaceDistanceMetric:
    """monai.metrics.SurfaceDistanceMetric's constructor and __call__(y_pred, y) with a `spacing=` keyword (no Cumulative
    buffering / aggregate())."""

    def __init__(self, include_background=False, symmetric=False, distance_metric="euclidean", reduction=None,
                 get_not_nans=False):
        _euclidean(distance_metric)
        self.include_background, self.symmetric, self.distance_metric = include_background, symmetric, distance_metric

    def __call__(self, y_pred, y, num_classes=None, label_values=MMWHS_LABEL_VALUES, spacing=None):
        return average_surface_distance(y_pred, y, num_classes, label_values, self.include_background, spacing, self.symmetric)


class SurfaceDiceMetric:
    """monai.metrics.SurfaceDiceMetric's constructor and __call__(y_pred, y) with a `spacing=` keyword (no Cumulative
    buffering / aggregate(), no use_subvoxels)."""

    def __init__(self, class_thresholds, include_background=False, distance_metric="euclidean", reduction=None,
                 get_not_nans=False):
        _euclidean(distance_metric)
        self.class_thresholds, self.include_background, self.distance_metric = class_thresholds, include_background, distance_metric

    def __call__(self, y_pred, y, num_classes=None, label_values=MMWHS_LABEL_VALUES, spacing=None):
        return surface_dice(y_pred, y, self.class_thresholds, num_classes, label_values, self.include_background, spacing)


__all__ = ["surface_distances", "workspace_bytes", "hausdorff_distance_mm", "average_surface_distance", "surface_dice",
           "SurfaceDistanceMetric", "SurfaceDiceMetric", "SurfaceDistances", "MMWHS_LABEL_VALUES", "SIGNATURES"]
