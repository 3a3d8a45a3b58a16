"""Test-time mirroring (nnU-Net's default at prediction time): the binding of include/micformer_mirror.h (kernels:
csrc/sliding_window.hip) and the host side of `inference.sliding_window_inference(mirror_axes=...)` and
`restore.segment_pair(mirror_axes=...)`.

    out = sliding_window_inference(x, 128, 7, model, mode="gaussian", mirror_axes=(0, 1, 2))
    logits = mirror.mirrored_logits(model, x, (0, 1, 2))                  # one whole-volume forward per flip, averaged

`mirror_axes` is a subset of {0, 1, 2} = (D, H, W), the spatial axes in nnU-Net's and RandFlipd's numbering.  A flip code is a 3-bit
mask (bit a set: axis a reversed); the flips of a call are all 2^k subsets of `mirror_axes` in ascending code order, code 0 first.
An item is (b, z0, y0, x0, f): a window and the flip it is predicted under.  Both flips of an item -- the window on the way in, its
prediction on the way back -- are index arithmetic inside the crop and the accumulate, so mirroring adds no pass over the data and
no buffer; the accumulate is the store-and-sum form of blend.py (one launch per item in list order, no float atomics).
"""
import torch

from . import _lib, blend

# name -> argument signature (as _lib.SIGNATURES)
SIGNATURES = {
    "micf_sw_mirror_window_batch": "pppiiiiiiiiip",
    "micf_sw_mirror_accumulate": "ppppiiiiiiiiipfp",
}
INT64_RETURNS = frozenset()

lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="test-time mirroring")


def flip_codes(mirror_axes):
    """Distinct ints from 0, 1, 2 (D, H, W) -> the flip codes of all their subsets, ascending; () -> [0]."""
    try:
        axes = list(mirror_axes)
    except TypeError:
        raise ValueError(f"mirror_axes must be a sequence of distinct axes from 0, 1, 2 (D, H, W), got {mirror_axes!r}") from None
    if isinstance(mirror_axes, (str, bytes)) or any(isinstance(a, bool) or not isinstance(a, int) or a not in (0, 1, 2) for a in axes) \
            or len(set(axes)) != len(axes):
        raise ValueError(f"mirror_axes must be a sequence of distinct axes from 0, 1, 2 (D, H, W), got {mirror_axes!r}")
    mask = sum(1 << a for a in axes)
    return [f for f in range(8) if f & ~mask == 0]


def window_batch(vol, items, roi):
    """vol [B, C, D, H, W]; items: a list of (b, z0, y0, x0, flip) -> [n, C, rd, rh, rw], window i cropped at its origin and reversed
    along the axes of its flip code; ONE launch."""
    B, C, D, H, W = vol.shape
    rd, rh, rw = roi
    win = torch.empty((len(items), C, rd, rh, rw), dtype=torch.float32, device=vol.device)
    _lib.call("micf_sw_mirror_window_batch", _lib.f32(vol), _lib.f32(win), _lib.int32_rows(items, 5), len(items), B, C, D, H, W,
              rd, rh, rw)
    return win


def accumulate(pred, out, wsum, items, taps=None, floor=1.0):
    """pred [n, K, rd, rh, rw], prediction i flipped back by its item's code and weighted into out [B, K, D, H, W] and wsum
    [B, D, H, W] at the item's window: one launch per item in list order, no atomics.  taps / floor: blend.device_taps(), or None
    for a weight of 1 (include/micformer_mirror.h)."""
    blend.store_and_sum("micf_sw_mirror_accumulate", 5, pred, out, wsum, items, taps, floor)


def mirrored_logits(model, x, mirror_axes):
    """x [B, C, D, H, W] float32 on the GPU, or a data.RawBatch without augmentation draws (the validation transform then runs inside
    the model, on the flipped raw image) -> the fp32 logits of model(x) averaged over the flips of `mirror_axes`:
    mean_f M_f(model(M_f(x))), the terms summed in code order.  One forward per code; the flipped input is one mirrored crop that
    covers the volume (code 0 is x itself), the prediction is flipped back inside the accumulate, micf_sw_normalize divides."""
    from .data import RawBatch
    codes = flip_codes(mirror_axes)
    raw = isinstance(x, RawBatch)
    if raw and x.params is not None:
        raise ValueError("mirrored_logits expects a RawBatch without augmentation draws (params=None)")
    if not raw and (not isinstance(x, torch.Tensor) or x.dim() != 5 or not x.is_cuda):
        raise ValueError("mirrored_logits expects a (B, C, D, H, W) CUDA (ROCm) tensor or a RawBatch")
    image = (x.image if raw else x).float().contiguous()           # (a float16 raw image widens exactly)
    B, _, D, H, W = image.shape
    out = wsum = None
    with torch.no_grad():
        for f in codes:
            items = [(b, 0, 0, 0, f) for b in range(B)]
            if f:
                flipped = window_batch(image, items, (D, H, W))
            pred = model((RawBatch(flipped) if raw else flipped) if f else x).float().contiguous()
            if out is None:
                if pred.dim() != 5 or pred.shape[0] != B or tuple(pred.shape[2:]) != (D, H, W):
                    raise ValueError(f"model returned {tuple(pred.shape)} for an input of {tuple(image.shape)}")
                out, wsum = blend.new_sums(B, pred.shape[1], D, H, W, image.device)
            accumulate(pred, out, wsum, items)
        blend.normalize(out, wsum)
    return out


__all__ = ["SIGNATURES", "accumulate", "flip_codes", "mirrored_logits", "window_batch"]
