"""On-device intensity augmentation: the binding of include/micformer_intensity.h (kernels: csrc/volume_intensity.hip) and the
host-side draw of its parameters.  The intensity half of nnU-Net's "moreDA" chain -- Gaussian noise, Gaussian blur, multiplicative
brightness, contrast, gamma -- on a batch that is already on the device:

    image, label_map, crop = loader.load_batch(samples)                           # [B, 2, 128, 128, 128] float16
    params, seeds = intensity.draw_intensity(len(samples), device="cuda")         # [B, 2, 8] float32, [B] int64
    intensity.augment_intensity(image, params, seeds, out=image)                  # in place

Every (sample, channel) is processed on its own, in batchgenerators' order; a step whose parameter is neutral is an exact no-op.
`params[b, c]` is {sigma, noise_std, brightness, contrast, gamma, gamma_mode, retain_stats, 0}; both tensors are read on the device
when the kernels run: a graph captured with `out=` picks up new draws after `params.copy_(...)` / `seeds.copy_(...)`.
Rules: include/micformer_intensity.h, DESIGN.md "Volume loader".
"""
import torch

from . import _args, _lib

F32, F16 = 0, 1                               # MICF_INTENSITY_*
DTYPES = {torch.float32: F32, torch.float16: F16}
MAX_CHANNELS = 4                              # MICF_INTENSITY_MAX_CHANNELS
MAX_VOLUMES = 65535                           # MICF_INTENSITY_MAX_VOLUMES (B * C)
SIGMA_RANGE = (0.1, 2.0)                      # of a sigma that is not 0
SLOTS = ("sigma", "noise_std", "brightness", "contrast", "gamma", "gamma_mode", "retain_stats", "reserved")
NEUTRAL = (0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0)
GAMMA_OFF, GAMMA_PLAIN, GAMMA_INVERTED = 0, 1, 2
STATS = ("mean", "min", "max", "m0", "s0", "power_mean", "power_std", "reserved")

# name -> argument signature (as _lib.SIGNATURES); the workspace query returns int64 (INT64_RETURNS), the other int
SIGNATURES = {
    "micf_intensity_augment_workspace": "iiiii",
    "micf_intensity_augment": "ppiiiiiippplpp",
}
INT64_RETURNS = frozenset(("micf_intensity_augment_workspace",))

lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="intensity augmentation")


def _typed(t, what, dtypes):
    names = " or ".join(str(d).replace("torch.", "") for d in dtypes)
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a {names} tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise TypeError(f"{what} must be a {names} tensor, got {t.dtype}")


def _placed(t, what, device):
    if not t.is_cuda:
        raise ValueError(f"micformer_amd.intensity runs on the GPU: {what} must be a CUDA (ROCm) tensor")
    if device is not None and t.device != device:
        raise ValueError(f"{what} must be on {device}, got {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def augment_intensity(image, params, seeds, out=None, return_stats=False):
    """image [B, C, D, H, W] float16 | float32 (C in 1..4), params [B, C, 8] float32, seeds [B] int64, all contiguous on one
    device -> the augmented batch, same shape and dtype (`out`, which may be `image`, or a new tensor); with return_stats also
    the float64 [B, C, 8] record {mean, min, max after the blur; m0, s0; mean, std after the power law; 0} of every channel.
    Every TypeError comes before the first ValueError, and nothing touches the device before the checks have passed."""
    _typed(image, "image", (torch.float16, torch.float32))
    _typed(params, "params", (torch.float32,))
    _typed(seeds, "seeds", (torch.int64,))
    if out is not None and not isinstance(out, torch.Tensor):
        raise TypeError(f"out must be a tensor or None, got {type(out).__name__}")
    shape = tuple(image.shape)
    if len(shape) != 5:
        raise ValueError(f"image must have shape [B, C, D, H, W], got {list(shape)}")
    B, C = shape[:2]
    if B < 1 or not 1 <= C <= MAX_CHANNELS or B * C > MAX_VOLUMES:
        raise ValueError(f"image needs at least one sample, 1..{MAX_CHANNELS} channels and at most {MAX_VOLUMES} (sample, channel) "
                         f"pairs, got {list(shape)}")
    D, H, W = _args.triple(shape[2:], "image's extents", max_extent=_args.MAX_EXTENT)
    if tuple(params.shape) != (B, C, len(SLOTS)):
        raise ValueError(f"params must have shape {[B, C, len(SLOTS)]}, got {list(params.shape)}")
    if tuple(seeds.shape) != (B,):
        raise ValueError(f"seeds must have shape {[B]}, got {list(seeds.shape)}")
    _placed(image, "image", None)
    _placed(params, "params", image.device)
    _placed(seeds, "seeds", image.device)
    if out is not None:
        _args.out_tensor(out, "out", shape, image.dtype, image.device)
    # ---- the device from here on
    if out is None:
        out = torch.empty_like(image)
    nbytes = _lib.query_bytes("micf_intensity_augment_workspace", B, C, D, H, W)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=image.device)
    stats = torch.empty(B, C, len(STATS), dtype=torch.float64, device=image.device) if return_stats else None
    _lib.call_on(image.device, "micf_intensity_augment", image.data_ptr(), out.data_ptr(), DTYPES[image.dtype], B, C, D, H, W,
                 params.data_ptr(), seeds.data_ptr(), workspace.data_ptr(), nbytes, None if stats is None else stats.data_ptr())
    return (out, stats) if return_stats else out


def _probability(p, what):
    if isinstance(p, bool) or not isinstance(p, (int, float)):
        raise TypeError(f"{what} must be a number, got {type(p).__name__}")
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"{what} must lie in [0, 1], got {p!r}")
    return float(p)


def _range(r, what, low=0.0, high=float("inf"), open_low=False):
    try:
        a, b = (float(v) for v in r)
    except (TypeError, ValueError):
        raise TypeError(f"{what} must be a pair of numbers, got {r!r}") from None
    if not (low <= a <= b <= high) or (open_low and a <= low):
        raise ValueError(f"{what} must be an ordered pair within [{low:g}, {high:g}], got {r!r}")
    return a, b


def _uniform(u, lo, hi):
    return lo + (hi - lo) * u


def _two_sided(side, u, lo, hi):
    """batchgenerators' draw of a contrast / gamma factor: with probability 1/2 (and a range that reaches below 1) uniform in
    [lo, 1), else uniform in [max(lo, 1), hi]."""
    below = (side < 0.5) & (lo < 1.0)
    return torch.where(below, _uniform(u, lo, 1.0), _uniform(u, max(lo, 1.0), hi))


def draw_intensity(batch, channels=2, generator=None, device="cpu", p_noise=0.1, noise_std=(0.0, 0.1), p_blur=0.2,
                   p_blur_channel=0.5, sigma=(0.5, 1.0), p_brightness=0.15, brightness=(0.75, 1.25), p_contrast=0.15,
                   contrast=(0.75, 1.25), gamma=(0.7, 1.5), p_gamma_inverted=0.1, p_gamma=0.3, retain_stats=True):
    """Random parameters of augment_intensity for a batch, drawn on the host from `generator` (as affine.draw_affine):
    -> (params [B, C, 8] float32, seeds [B] int64) on `device`.  The defaults are the ranges and probabilities of nnU-Net's
    "moreDA" chain (data_augmentation_moreDA.py):

      noise       per sample with p 0.1: std uniform in (0, 0.1), one value for the channels of the sample
      blur        per sample with p 0.2, then per channel with p 0.5: sigma uniform in (0.5, 1), a value per channel
      brightness  per sample with p 0.15: a factor uniform in (0.75, 1.25) per channel
      contrast    per sample with p 0.15: a factor per channel from (0.75, 1.25) by batchgenerators' two-sided draw (half the
                  time uniform below 1, else uniform above)
      gamma       per sample inverted with p 0.1, else plain with p 0.3; the exponent per channel from (0.7, 1.5) by the same
                  two-sided draw; retain_stats on
    A step that is not drawn gets its neutral value (sigma 0, std 0, factor 1, gamma 1 with mode 0 and retain_stats 0).  A sigma
    range must lie in [0.1, 2.0], the range the kernels implement.

    Parity with batchgenerators is unpinned: the library was not available to compare against, so the order in which the random
    numbers are consumed, and with it the stream of draws for a given seed, is this function's own; only the distributions above
    are batchgenerators'.  moreDA applies GammaTransform twice per sample (inverted with p 0.1, then plain with p 0.3); here ONE
    gamma stage per sample replaces its two, so the 3 % of samples that moreDA would put through both get the inverted one only."""
    if isinstance(batch, bool) or not isinstance(batch, int):
        raise TypeError(f"batch must be an integer, got {type(batch).__name__}")
    if isinstance(channels, bool) or not isinstance(channels, int):
        raise TypeError(f"channels must be an integer, got {type(channels).__name__}")
    probs = [_probability(p, n) for p, n in ((p_noise, "p_noise"), (p_blur, "p_blur"), (p_blur_channel, "p_blur_channel"),
                                             (p_brightness, "p_brightness"), (p_contrast, "p_contrast"),
                                             (p_gamma_inverted, "p_gamma_inverted"), (p_gamma, "p_gamma"))]
    p_noise, p_blur, p_blur_channel, p_brightness, p_contrast, p_gamma_inverted, p_gamma = probs
    noise_std = _range(noise_std, "noise_std")
    brightness = _range(brightness, "brightness", open_low=True)
    contrast = _range(contrast, "contrast", open_low=True)
    gamma = _range(gamma, "gamma", open_low=True)
    sigma = _range(sigma, "sigma", *SIGMA_RANGE)
    if batch < 1:
        raise ValueError(f"batch must be at least 1, got {batch}")
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"channels must lie in 1..{MAX_CHANNELS}, got {channels}")
    gate = torch.rand(batch, 6, generator=generator, dtype=torch.float64)          # noise, blur, brightness, contrast, inverted, plain
    per = torch.rand(batch, channels, 8, generator=generator, dtype=torch.float64)
    std = torch.rand(batch, generator=generator, dtype=torch.float64)
    seeds = torch.randint(-2 ** 63, 2 ** 63 - 1, (batch,), generator=generator, dtype=torch.int64)
    on = lambda g: g[:, None].expand(batch, channels)                              # noqa: E731
    zero, one = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)
    params = torch.zeros(batch, channels, len(SLOTS), dtype=torch.float64)
    blur = on(gate[:, 1] < p_blur) & (per[:, :, 0] < p_blur_channel)
    params[:, :, 0] = torch.where(blur, _uniform(per[:, :, 1], *sigma), zero)
    params[:, :, 1] = torch.where(on(gate[:, 0] < p_noise), on(_uniform(std, *noise_std)), zero)
    params[:, :, 2] = torch.where(on(gate[:, 2] < p_brightness), _uniform(per[:, :, 2], *brightness), one)
    params[:, :, 3] = torch.where(on(gate[:, 3] < p_contrast), _two_sided(per[:, :, 3], per[:, :, 4], *contrast), one)
    inverted = on(gate[:, 4] < p_gamma_inverted)
    plain = ~inverted & on(gate[:, 5] < p_gamma)
    params[:, :, 4] = torch.where(inverted | plain, _two_sided(per[:, :, 5], per[:, :, 6], *gamma), one)
    params[:, :, 5] = torch.where(inverted, 2 * one, torch.where(plain, one, zero))
    params[:, :, 6] = torch.where(inverted | plain, one if retain_stats else zero, zero)
    params = params.to(torch.float32)
    s = params[:, :, 0]
    s[(s > 0) & (s < SIGMA_RANGE[0])] = SIGMA_RANGE[0]                             # (the float32 rounding of a range's end)
    s[s > SIGMA_RANGE[1]] = SIGMA_RANGE[1]
    return params.contiguous().to(device), seeds.to(device)


__all__ = ["DTYPES", "NEUTRAL", "SIGNATURES", "SLOTS", "STATS", "augment_intensity", "draw_intensity"]
