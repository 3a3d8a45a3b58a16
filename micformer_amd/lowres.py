"""On-device low-resolution simulation: the binding of include/micformer_lowres.h (kernels: csrc/volume_lowres.hip) and the
host-side draw of its targets.  batchgenerators' SimulateLowResolutionTransform as nnU-Net's "moreDA" chain configures it -- a
nearest-neighbour downsample of a channel to a random fraction of its extents and a cubic B-spline upsample back -- on a batch
that is already on the device, and `augment_moreda`, the intensity chain with this step at moreDA's place:

    image, label_map, crop = loader.load_batch(samples)                           # [B, 2, 128, 128, 128] float16
    params, seeds = intensity.draw_intensity(len(samples), device="cuda")
    target = lowres.draw_low_resolution(len(samples), image.shape[2:], device="cuda")   # [B, 2, 3] int32
    lowres.augment_moreda(image, params, seeds, target, out=image)                # in place

`target[b, c]` is the low-resolution grid (td, th, tw) of the channel; a channel whose target equals the image's extents is off and
comes back bit for bit.  The tensor is read on the device when the kernels run: a graph captured with `out=` picks up new draws
after `target.copy_(...)`.  Only this configuration (order 0 down, order 3 up, edge boundary) is offered.
Rules: include/micformer_lowres.h, DESIGN.md "Low-resolution simulation".
"""
import numpy as np
import torch

from . import _args, _lib, intensity

F32, F16 = 0, 1                               # MICF_LOWRES_*
DTYPES = {torch.float32: F32, torch.float16: F16}
MAX_CHANNELS = 4                              # MICF_LOWRES_MAX_CHANNELS
MAX_VOLUMES = 65535                           # MICF_LOWRES_MAX_VOLUMES (B * C)

# name -> argument signature (as _lib.SIGNATURES); the workspace query returns int64 (INT64_RETURNS), the other int
SIGNATURES = {
    "micf_lowres_workspace": "iiiii",
    "micf_lowres_simulate": "ppiiiiiipplp",
}
INT64_RETURNS = frozenset(("micf_lowres_workspace",))

lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="low-resolution simulation")


def _typed(t, what, dtypes):
    names = " or ".join(str(d).replace("torch.", "") for d in dtypes)
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a {names} tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise TypeError(f"{what} must be a {names} tensor, got {t.dtype}")


def _placed(t, what, device):
    if not t.is_cuda:
        raise ValueError(f"micformer_amd.lowres runs on the GPU: {what} must be a CUDA (ROCm) tensor")
    if device is not None and t.device != device:
        raise ValueError(f"{what} must be on {device}, got {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def _checked(image, target, out):
    """Types, then shapes: every TypeError before the first ValueError, nothing on the device.  -> shape"""
    _typed(image, "image", (torch.float16, torch.float32))
    _typed(target, "target", (torch.int32,))
    if out is not None and not isinstance(out, torch.Tensor):
        raise TypeError(f"out must be a tensor or None, got {type(out).__name__}")
    shape = tuple(image.shape)
    if len(shape) != 5:
        raise ValueError(f"image must have shape [B, C, D, H, W], got {list(shape)}")
    B, C = shape[:2]
    if B < 1 or not 1 <= C <= MAX_CHANNELS or B * C > MAX_VOLUMES:
        raise ValueError(f"image needs at least one sample, 1..{MAX_CHANNELS} channels and at most {MAX_VOLUMES} (sample, channel) "
                         f"pairs, got {list(shape)}")
    _args.triple(shape[2:], "image's extents", max_extent=_args.MAX_EXTENT)
    if tuple(target.shape) != (B, C, 3):
        raise ValueError(f"target must have shape {[B, C, 3]}, got {list(target.shape)}")
    return shape


def _on_device(image, target, out):
    _placed(image, "image", None)
    _placed(target, "target", image.device)
    if out is not None:
        _args.out_tensor(out, "out", tuple(image.shape), image.dtype, image.device)


def simulate_low_resolution(image, target, out=None):
    """image [B, C, D, H, W] float16 | float32 (C in 1..4), target [B, C, 3] int32 (td, th, tw), both contiguous on one device ->
    every channel downsampled to its target by nearest neighbour and upsampled back by cubic B-spline interpolation, same shape
    and dtype (`out`, which may be `image`, or a new tensor).  The device clamps a target value into [1, extent]; a channel whose
    target equals the extents is returned bit for bit.  Cubic overshoot is kept.  Every TypeError comes before the first
    ValueError, and nothing touches the device before the checks have passed."""
    B, C, D, H, W = _checked(image, target, out)
    _on_device(image, target, out)
    # ---- the device from here on
    if out is None:
        out = torch.empty_like(image)
    nbytes = _lib.query_bytes("micf_lowres_workspace", B, C, D, H, W)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=image.device)
    _lib.call_on(image.device, "micf_lowres_simulate", image.data_ptr(), out.data_ptr(), DTYPES[image.dtype], B, C, D, H, W,
                 target.data_ptr(), workspace.data_ptr(), nbytes)
    return out


def draw_low_resolution(batch, size, channels=2, generator=None, device="cpu", p_per_sample=0.25, p_per_channel=0.5,
                        zoom_range=(0.5, 1.0), ignore_axes=()):
    """Random targets of simulate_low_resolution for a batch of volumes of extents `size` = (D, H, W), drawn on the host from
    `generator` (as intensity.draw_intensity): -> int32 [B, C, 3] on `device`.  The defaults are those of nnU-Net's "moreDA" chain:

      per sample with p 0.25, then per channel with p 0.5: a zoom uniform in (0.5, 1) per channel,
      t = np.round(size * zoom) per axis (half to even, as numpy rounds), clamped to [1, size]; an axis in `ignore_axes`
      (0, 1, 2 for D, H, W) keeps t = size, and so does every axis of a channel that is not drawn: it is off.

    Parity with batchgenerators is unpinned: the library was not available to compare against, so the order in which the random
    numbers are consumed, and with it the stream of draws for a given seed, is this function's own; only the distribution above
    is batchgenerators'."""
    if isinstance(batch, bool) or not isinstance(batch, int):
        raise TypeError(f"batch must be an integer, got {type(batch).__name__}")
    if isinstance(channels, bool) or not isinstance(channels, int):
        raise TypeError(f"channels must be an integer, got {type(channels).__name__}")
    p_per_sample = intensity._probability(p_per_sample, "p_per_sample")
    p_per_channel = intensity._probability(p_per_channel, "p_per_channel")
    zoom_range = intensity._range(zoom_range, "zoom_range", open_low=True)
    try:
        ignore = tuple(ignore_axes)
    except TypeError:
        raise TypeError(f"ignore_axes must be a sequence of axes, got {ignore_axes!r}") from None
    if any(isinstance(a, bool) or not isinstance(a, int) for a in ignore):
        raise TypeError(f"ignore_axes must be a sequence of integers, got {ignore_axes!r}")
    size = _args.triple(size, "size", max_extent=_args.MAX_EXTENT)
    if batch < 1:
        raise ValueError(f"batch must be at least 1, got {batch}")
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"channels must lie in 1..{MAX_CHANNELS}, got {channels}")
    if any(not 0 <= a <= 2 for a in ignore):
        raise ValueError(f"ignore_axes must name axes 0, 1 or 2 of (D, H, W), got {ignore_axes!r}")
    gate = torch.rand(batch, generator=generator, dtype=torch.float64)
    per = torch.rand(batch, channels, 2, generator=generator, dtype=torch.float64)
    on = ((gate[:, None] < p_per_sample) & (per[:, :, 0] < p_per_channel)).numpy()
    zoom = intensity._uniform(per[:, :, 1], *zoom_range).numpy()
    full = np.array(size, np.float64)
    t = np.clip(np.round(full[None, None, :] * zoom[:, :, None]), 1.0, full)
    keep = np.zeros(3, bool)
    keep[list(ignore)] = True
    t = np.where(on[:, :, None] & ~keep[None, None, :], t, full)
    return torch.from_numpy(t.astype(np.int32)).contiguous().to(device)


GAMMA_SLOTS = slice(4, 7)                     # gamma, gamma_mode, retain_stats of intensity.SLOTS


def augment_moreda(image, params, seeds, target, out=None):
    """moreDA's order of the intensity transforms with the low-resolution step in its place, between contrast and gamma:
    augment_intensity with the gamma slots neutral, simulate_low_resolution, augment_intensity with the gamma slots alone (a step
    of augment_intensity that is off is an exact no-op).  Arguments as augment_intensity's and simulate_low_resolution's.  For a
    float32 image this is the single float32 chain with the step inserted; for a float16 image the two hand-overs add two float16
    roundings to the one at the end.  With every target off the result is that of the two augment_intensity calls alone."""
    intensity._typed(params, "params", (torch.float32,))           # (the TypeErrors of all three calls before any ValueError)
    intensity._typed(seeds, "seeds", (torch.int64,))
    B, C = _checked(image, target, out)[:2]
    if tuple(params.shape) != (B, C, len(intensity.SLOTS)):
        raise ValueError(f"params must have shape {[B, C, len(intensity.SLOTS)]}, got {list(params.shape)}")
    if tuple(seeds.shape) != (B,):
        raise ValueError(f"seeds must have shape {[B]}, got {list(seeds.shape)}")
    _on_device(image, target, out)
    intensity._placed(params, "params", image.device)
    intensity._placed(seeds, "seeds", image.device)
    # ---- the device from here on
    neutral =torch.tensor(intensity.NEUTRAL, dtype=torch.float32, device=params.device)
    first, last = params.clone(), neutral.expand_as(params).contiguous()
    first[..., GAMMA_SLOTS] = neutral[GAMMA_SLOTS]
    last[..., GAMMA_SLOTS] = params[..., GAMMA_SLOTS]
    out = intensity.augment_intensity(image, first, seeds, out=out)
    simulate_low_resolution(out, target, out=out)
    return intensity.augment_intensity(out, last, seeds, out=out)


__all__ = ["DTYPES", "SIGNATURES", "augment_moreda", "draw_low_resolution", "simulate_low_resolution"]
