"""On-device evaluation metrics of the reference's test notebook: percentile Hausdorff distance (HD95) and mean IoU, restated
from MONAI 1.1 (monai.metrics.HausdorffDistanceMetric / MeanIoU) on the HIP kernels of csrc/surface_metrics.hip.

    from micformer_amd.metrics import HausdorffDistanceMetric, MeanIoU
    hd95 = HausdorffDistanceMetric(include_background=False, percentile=95)(y_pred, y)    # float32 [B, K-1] on the device

Inputs are either uint8 class maps [B, D, H, W] (num_classes required) or one-hot planes [B, K, D, H, W] of any dtype (cast
with .float() as MONAI does; a voxel is in class c where the plane equals 1.0).  Nothing here synchronises with the host.
The entry points are declared in include/micformer_metrics.h; _lib.bind binds them from this module's table (SIGNATURES below),
which is apart from include/micformer_hip.h's.
"""
import torch

from . import _lib

FORM_LABEL, FORM_ONEHOT = 0, 1

# name -> argument signature (as _lib.SIGNATURES); the two *_workspace queries return int64 (INT64_RETURNS), the others int
SIGNATURES = {
    "micf_surface_metrics_workspace": "iiiii",
    "micf_hausdorff_distance": "ppiiiiiiidiplpp",
    "micf_mean_iou_workspace": "iiiii",
    "micf_mean_iou": "ppiiiiiiiiplpp",
}
INT64_RETURNS = frozenset(("micf_surface_metrics_workspace", "micf_mean_iou_workspace"))

lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="surface metrics")


def _inputs(y_pred, y, num_classes):
    """-> (pred, gt, form, B, K, D, H, W) with both tensors contiguous on the device in the kernels' form."""
    if not isinstance(y_pred, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise TypeError("y_pred and y must be tensors")
    if not (y_pred.is_cuda and y.is_cuda):
        raise ValueError("micformer_amd.metrics runs on the GPU: y_pred and y must be CUDA (ROCm) tensors")
    if y_pred.shape != y.shape:
        raise ValueError(f"y_pred and y must have the same shape, got {tuple(y_pred.shape)} and {tuple(y.shape)}")
    if y_pred.dim() == 4:
        if y_pred.dtype != torch.uint8 or y.dtype != torch.uint8:
            raise TypeError("a 4-D input is a class map and must be uint8")
        if num_classes is None:
            raise ValueError("class-map inputs need num_classes")
        K = int(num_classes)
        B, D, H, W = y_pred.shape
        return y_pred.contiguous(), y.contiguous(), FORM_LABEL, B, K, D, H, W
    if y_pred.dim() == 5:
        B, K, D, H, W = y_pred.shape
        if num_classes is not None and int(num_classes) != K:
            raise ValueError(f"num_classes={num_classes} does not match the {K} planes")
        return y_pred.float().contiguous(), y.float().contiguous(), FORM_ONEHOT, B, K, D, H, W
    raise ValueError(f"expected a uint8 class map [B, D, H, W] or one-hot planes [B, K, D, H, W], got {y_pred.dim()}-D")


def _first_class(include_background, K):
    first = 0 if include_background else 1
    if first >= K:
        raise ValueError("include_background=False needs at least two classes")
    return first


def hausdorff_distance(y_pred, y, num_classes=None, include_background=False, percentile=None, directed=False,
                       distance_metric="euclidean"):
    """MONAI 1.1 compute_hausdorff_distance on the device: float32 [B, K'] in voxel units (nan where both edge sets are empty,
    +inf where exactly one is).  percentile None or 0 = the maximum."""
    if distance_metric != "euclidean":
        raise ValueError(f"distance_metric {distance_metric!r} is not implemented (only 'euclidean')")
    p = 0.0 if not percentile else float(percentile)
    if not 0.0 <= p <= 100.0:
        raise ValueError(f"percentile should be a value between 0 and 100, got {percentile}")
    pred, gt, form, B, K, D, H, W = _inputs(y_pred, y, num_classes)
    first = _first_class(include_background, K)
    nbytes = _lib.query_bytes("micf_surface_metrics_workspace", B, K, D, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    out = torch.empty((B, K - first), dtype=torch.float32, device=pred.device)
    _lib.call_on(pred.device, "micf_hausdorff_distance", pred.data_ptr(), gt.data_ptr(), form, B, K, D, H, W, first, p,
                 1 if directed else 0, ws.data_ptr(), nbytes, out.data_ptr())
    return out


def mean_iou(y_pred, y, num_classes=None, include_background=False, ignore_empty=True):
    """MONAI 1.1 compute_iou on the device: float32 [B, K'] from exact integer counts."""
    pred, gt, form, B, K, D, H, W = _inputs(y_pred, y, num_classes)
    first = _first_class(include_background, K)
    nbytes = _lib.query_bytes("micf_mean_iou_workspace", B, K, D, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    out = torch.empty((B, K - first), dtype=torch.float32, device=pred.device)
    _lib.call_on(pred.device, "micf_mean_iou", pred.data_ptr(), gt.data_ptr(), form, B, K, D, H, W, first, 1 if ignore_empty else 0,
                 ws.data_ptr(), nbytes, out.data_ptr())
    return out


class HausdorffDistanceMetric:
    """monai.metrics.HausdorffDistanceMetric's constructor and __call__(y_pred, y) (no Cumulative buffering / aggregate())."""

    def __init__(self, include_background=False, distance_metric="euclidean", percentile=None, directed=False,
                 reduction=None, get_not_nans=False):
        if distance_metric != "euclidean":
            raise ValueError(f"distance_metric {distance_metric!r} is not implemented (only 'euclidean')")
        if percentile and not 0 <= percentile <= 100:
            raise ValueError(f"percentile should be a value between 0 and 100, got {percentile}")
        self.include_background, self.distance_metric = include_background, distance_metric
        self.percentile, self.directed = percentile, directed

    def __call__(self, y_pred, y, num_classes=None):
        return hausdorff_distance(y_pred, y, num_classes=num_classes, include_background=self.include_background,
                                  percentile=self.percentile, directed=self.directed, distance_metric=self.distance_metric)


class MeanIoU:
    """monai.metrics.MeanIoU's constructor and __call__(y_pred, y) (no Cumulative buffering / aggregate())."""

    def __init__(self, include_background=True, reduction=None, get_not_nans=False, ignore_empty=True):
        self.include_background, self.ignore_empty = include_background, ignore_empty

    def __call__(self, y_pred, y, num_classes=None):
        return mean_iou(y_pred, y, num_classes=num_classes, include_background=self.include_background,
                        ignore_empty=self.ignore_empty)


__all__ = ["hausdorff_distance", "mean_iou", "HausdorffDistanceMetric", "MeanIoU", "SIGNATURES"]
