"""The referee of sliding-window inference with test-time mirroring (micformer_amd.inference mirror_axes=, micformer_amd/mirror.py),
built on tests/sw_blend_ref.py: the whole blend in float64 from the float32 importance map and the float32 per-ITEM predictions
handed to it -- so a GPU test feeds it the device's own predictions and the only error left is the blend's.

Definition (include/micformer_mirror.h, DESIGN.md "Sliding-window inference"): mirror_axes is a subset of {0, 1, 2} = (D, H, W); a
flip code f is a 3-bit mask, bit a set = axis a reversed; the flips of a call are all subsets of mirror_axes in ascending code
order; M_f reverses the window index along the set axes; p_{i,f} = predictor(M_f(window_i)) and
    out[b, k, v] = sum_i sum_f w_i(v) p_{i,f}[k, M_f(v - o_i)] / sum_i sum_f w_i(v)
over the windows i that cover v, w the map of sw_blend_ref.importance_map (ones for mode="constant").  Items are enumerated
window-major: (window 0, code 0), (window 0, next code), ...

`mutate` builds the wrong referees that tests/test_sw_mirror_cpu.py shows the bound to reject."""
import torch

import sw_blend_ref as S

MUTATIONS = ("no_unflip", "swap_bits", "drop_flip", "one_weight_per_window")


def flip_codes(mirror_axes):
    mask = sum(1 << a for a in mirror_axes)
    return [f for f in range(8) if f & ~mask == 0]


def flip(t, code):
    """t [..., d, h, w] reversed along the spatial axes whose bit is set in `code`."""
    dims = [a - 3 for a in range(3) if code >> a & 1]
    return t.flip(dims) if dims else t


def items(shape, roi, overlap, mirror_axes):
    """[(b, z0, y0, x0, f)] in the order micformer_amd.inference enumerates them: the windows of sw_blend_ref.plan, each under
    every flip code in ascending order."""
    return [w + (f,) for w in S.plan(shape, roi, overlap)[2] for f in flip_codes(mirror_axes)]


def crops(x, roi, overlap, mirror_axes):
    """M_f(window_i) in items() order: a list of [1, C, rd, rh, rw] tensors."""
    codes = flip_codes(mirror_axes)
    return [flip(c, f).contiguous() for c in S.crops(x, roi, overlap) for f in codes]


def blend(shape, preds, roi, overlap, mirror_axes, mode="gaussian", sigma_scale=0.125, mutate=None):
    """shape: the (B, C, D, H, W) of the input volume; preds: one float32 [1, K, rd, rh, rw] (or [K, rd, rh, rw]) prediction per
    item in items() order -> float64 [B, K, D, H, W]."""
    assert mutate is None or mutate in MUTATIONS
    pads, padded, _ = S.plan(shape, roi, overlap)
    its = items(shape, roi, overlap, mirror_axes)
    codes = flip_codes(mirror_axes)
    assert len(preds) == len(its)
    wmap, _ = S.importance_map(roi, mode, sigma_scale)
    w = wmap.double()
    K = preds[0].shape[-4]
    num = torch.zeros((shape[0], K) + padded, dtype=torch.float64)
    den = torch.zeros((shape[0],) + padded, dtype=torch.float64)
    middle = (len(its) // len(codes) // 2) * len(codes) + len(codes) - 1          # the last flip of the middle window
    for i, ((b, z, y, x, f), p) in enumerate(zip(its, preds)):
        assert p.dtype == torch.float32
        if mutate == "drop_flip" and i == middle:
            continue
        back = f
        if mutate == "no_unflip":
            back = 0
        elif mutate == "swap_bits":
            back = (f & 2) | (f & 1) << 2 | (f & 4) >> 2
        p = flip(p.reshape((K,) + tuple(roi)), back).double()
        num[b, :, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += w * p
        if mutate != "one_weight_per_window" or f == 0:
            den[b, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += w
    out = num / den[:, None]
    (pd, ph, pw), (D, H, W) = pads, shape[2:]
    return out[:, :, pd // 2:pd // 2 + D, ph // 2:ph // 2 + H, pw // 2:pw // 2 + W]


def sliding_window(x, predictor, roi, overlap, mirror_axes, **kw):
    """The predictor run here, item by item (a CPU predictor for the CPU tests)."""
    return blend(x.shape, [predictor(c).float() for c in crops(x, roi, overlap, mirror_axes)], roi, overlap, mirror_axes, **kw)


def bound(shape, roi, overlap, mirror_axes, preds):
    """-> (the derived bound, n_max, F).  As sw_blend_ref.bound with n_max * F terms on the busiest voxel (F = 2^k flips of each of
    the n_max windows): at most 2 n F roundings in the numerator, n F in the denominator and one in the division:
    |got - ref| <= (3 n_max F + 2) * 2^-24 * max|p|."""
    n_max = int(S.visits(shape, roi, overlap).max())
    F = len(flip_codes(mirror_axes))
    p_max = max(float(p.abs().max()) for p in preds)
    return (3 * n_max * F + 2) * 2.0 ** -24 * p_max, n_max, F
