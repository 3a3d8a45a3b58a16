"""Importance maps and the weighted accumulate of sliding-window inference: the binding of include/micformer_blend.h (kernels:
csrc/sliding_window.hip) and the host side of `inference.sliding_window_inference(mode="gaussian")`.

    w = blend.importance_map((128, 128, 128), "gaussian", sigma_scale=0.125)        # float32 [rd, rh, rw]

The Gaussian map restates MONAI's `compute_importance_map(mode="gaussian")` in its separable closed form (MONAI itself is not
available to compare against: parity with it is UNPINNED, this definition is the referee; DESIGN.md "Sliding-window inference").
Per axis i of n_i voxels, sigma_i = sigma_scale_i * n_i and, in float32 on the host,
    g_i[j] = exp(-(j - (n_i - 1) / 2)^2 / (2 sigma_i^2)),     m = (g_0[:, None] * g_1[None, :])[:, :, None] * g_2,
    floor = max(min(m), 1e-3),                                 map = max(m, floor).
The host builds the three tap vectors and `floor`; the device rebuilds max((g0[z] * g1[y]) * g2[x], floor) with the same two float32
multiplies, so its weights are bit-equal to `importance_map()`.
"""
import math

import torch

from . import _lib

MODES = ("constant", "gaussian")
FLOOR = 1e-3

# name -> argument signature (as _lib.SIGNATURES)
SIGNATURES = {
    "micf_sw_blend_accumulate": "ppppiiiiiiiiipfp",
}
INT64_RETURNS = frozenset()

lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="Gaussian blending")


def check_mode(mode):
    """"constant" | "gaussian"; any other mode of MONAI's inferer is not implemented."""
    if mode not in MODES:
        raise NotImplementedError(f"mode must be one of {list(MODES)} (MONAI's default and its Gaussian blending), got {mode!r}")
    return mode


def roi3(roi_size):
    """An int (for all three axes) or a (rd, rh, rw) triple of positive ints -> three ints."""
    if isinstance(roi_size, int) and not isinstance(roi_size, bool):
        roi_size = (roi_size,) * 3
    roi = tuple(int(r) for r in roi_size)
    if len(roi) != 3 or any(r < 1 for r in roi):
        raise ValueError(f"roi_size must be a positive int or three of them, got {roi_size!r}")
    return roi


def sigma_scales(sigma_scale):
    """A positive float (for all three axes) or three of them, one per axis -> three floats; anything else is a ValueError."""
    try:
        vals = [float(v) for v in sigma_scale] if hasattr(sigma_scale, "__len__") else [float(sigma_scale)] * 3
    except (TypeError, ValueError):
        raise ValueError(f"sigma_scale must be a positive float or three of them, got {sigma_scale!r}") from None
    if isinstance(sigma_scale, (str, bytes, bool)) or len(vals) != 3 or not all(math.isfinite(v) and v > 0.0 for v in vals):
        raise ValueError(f"sigma_scale must be a positive float or three of them (one per axis), got {sigma_scale!r}")
    return vals


def gaussian_taps(roi_size, sigma_scale=0.125):
    """-> ([g0, g1, g2] float32 host vectors of rd, rh, rw entries, floor as a Python float that float32 holds exactly)."""
    roi, scales = roi3(roi_size), sigma_scales(sigma_scale)
    taps = []
    for n, s in zip(roi, scales):
        sigma = s * n
        j = torch.arange(n, dtype=torch.float32)
        taps.append(torch.exp(-((j - (n - 1) / 2.0) ** 2) / (2.0 * sigma * sigma)))
    m = (taps[0][:, None] * taps[1][None, :])[:, :, None] * taps[2]
    floor = torch.tensor(max(float(m.min()), FLOOR), dtype=torch.float32)
    return taps, float(floor)


def importance_map(roi_size, mode="constant", sigma_scale=0.125, device=None):
    """The weight of every voxel of a window: float32 [rd, rh, rw] on `device` (the host by default).  "constant": ones (sigma_scale
    is ignored); "gaussian": the map of this module's header, the very weights the device applies."""
    check_mode(mode)
    roi = roi3(roi_size)
    if mode == "constant":
        return torch.ones(roi, dtype=torch.float32, device=device)
    taps, floor = gaussian_taps(roi, sigma_scale)
    m = (taps[0][:, None] * taps[1][None, :])[:, :, None] * taps[2]
    m = torch.maximum(m, torch.tensor(floor, dtype=torch.float32))
    return m if device is None else m.to(device)


def device_taps(roi_size, sigma_scale, device):
    """-> (g0 | g1 | g2 as one float32 tensor of rd + rh + rw entries on `device`, floor): the `taps` / `floor` arguments of
    accumulate()."""
    taps, floor = gaussian_taps(roi_size, sigma_scale)
    return torch.cat(taps).to(device).contiguous(), floor


def store_and_sum(entry, width, pred, out, wsum, items, taps, floor):
    """The store-and-sum accumulate behind accumulate() and mirror.accumulate(): C entry point `entry`, whose items have `width`
    ints; taps None: no taps."""
    B, K, D, H, W = out.shape
    rd, rh, rw = pred.shape[2:]
    if pred.shape[0] != len(items) or pred.shape[1] != K or tuple(wsum.shape) != (B, D, H, W) or \
            (taps is not None and taps.numel() != rd + rh + rw):
        raise ValueError(f"{entry}: pred {tuple(pred.shape)}, out {tuple(out.shape)}, wsum {tuple(wsum.shape)}, {len(items)} items "
                         f"and {'no' if taps is None else taps.numel()} taps do not fit together")
    _lib.call(entry, _lib.f32(pred), _lib.f32(out), _lib.f32(wsum), _lib.int32_rows(items, width), len(items), B, K, D, H, W,
              rd, rh, rw, _lib.f32(taps), floor)


def accumulate(pred, out, wsum, chunk, taps, floor):
    """pred [n, K, rd, rh, rw] weighted into out [B, K, D, H, W] and wsum [B, D, H, W] at the windows of `chunk` (a list of
    (b, z0, y0, x0)): one launch per window in list order, no atomics (include/micformer_blend.h)."""
    store_and_sum("micf_sw_blend_accumulate", 4, pred, out, wsum, chunk, taps, floor)


def new_sums(B, K, D, H, W, device, reuse=None):
    """-> (out [B, K, D, H, W], wsum [B, D, H, W]): the float32 sums of a volume, zeroed (one memset node each); `reuse`: a pair
    of these shapes to zero and return instead of a new one."""
    out, wsum = reuse or (torch.empty((B, K, D, H, W), dtype=torch.float32, device=device),
                          torch.empty((B, D, H, W), dtype=torch.float32, device=device))
    for t in (out, wsum):
        _lib.call("micf_zero", _lib.ptr(t), t.numel() * 4)
    return out, wsum


def normalize(out, wsum):
    """out[b, k, v] /= wsum[b, v] in place: micf_sw_normalize, one launch per sample."""
    for o, w in zip(out, wsum):
        _lib.call("micf_sw_normalize", _lib.f32(o), _lib.f32(w), o.shape[0], w.numel())


__all__ = ["MODES", "SIGNATURES", "accumulate", "check_mode", "device_taps", "gaussian_taps", "importance_map", "new_sums",
           "normalize", "sigma_scales", "store_and_sum"]
