"""Referee of the volume restore (micformer_amd/restore.py): torch's own operators on whatever device the logits live on (the CPU
in every test but the full-size one) -- F.interpolate(mode="trilinear", align_corners=False) of the logits or of their softmax, then
argmax and the class -> label value lookup -- plus the per-voxel top-1 minus top-2 MARGIN that the acceptance rule needs.

Acceptance rule (`judge`): where the referee's margin >= tau the device label must equal the referee's; where it is < tau (a near
tie) the device label must be a class whose referee value lies within tau of the maximum.  tau = 1e-4 for logits, 1e-5 for
probabilities: eight fp32 products of magnitude <= 12 are within about 8 * 2^-24 * 12 ~ 6e-6 of exact (the referee against
float64, on 9x14x11 -> 20x33x27 of tests/test_restore_cpu.py: 2.2e-6 for logits, 3.2e-7 for probabilities), tau is 10 - 20 times
that.  The share of near-tie voxels is a CONDITION of a test case, at most MAX_NEAR_TIE_SHARE, asserted on the referee alone before
the device is asked.
"""
import numpy as np
import torch
import torch.nn.functional as F

MMWHS_LABEL_VALUES = (205, 420, 500, 550, 600, 820, 850)
TAU = {False: 1e-4, True: 1e-5}            # keyed by `probabilities`
MAX_NEAR_TIE_SHARE = 5e-4


def make_logits(src, K=8, batch=1, noise=0.3, seed=0):
    """The input recipe: smooth class fields (|logits| <= about 12) plus a little noise.  -> [batch, K, *src] float32 on the CPU."""
    torch.manual_seed(seed)
    base = torch.randn(batch, K, 6, 6, 6)
    return (3 * F.interpolate(base, size=tuple(src), mode="trilinear") + noise * torch.randn(batch, K, *src)).contiguous()


def label_table(label_values, K, device="cpu"):
    """class -> stored value: the class itself with label_values None, else 0 and the K - 1 label values."""
    if label_values is None:
        return torch.arange(K, dtype=torch.int64, device=device)
    assert len(label_values) == K - 1
    return torch.tensor([0] + [int(v) for v in label_values], dtype=torch.int64, device=device)


def upsample(logits, shape, probabilities=False):
    """logits [K, D, H, W] -> the interpoland at `shape`, [K, d, h, w] float32."""
    x = logits.float()
    if probabilities:
        x = torch.softmax(x, 0)
    return F.interpolate(x[None], size=tuple(int(s) for s in shape), mode="trilinear", align_corners=False)[0]


def margin_of(up):
    """top-1 minus top-2 over the classes, +inf for a single class."""
    if up.shape[0] == 1:
        return torch.full(up.shape[1:], float("inf"), device=up.device)
    top = up.topk(2, dim=0).values
    return top[0] - top[1]


def restore(logits, shape, label_values=MMWHS_LABEL_VALUES, probabilities=False):
    """-> (labels int64 [d, h, w], margin float32 [d, h, w], the upsampled interpoland [K, d, h, w])."""
    up = upsample(logits, shape, probabilities)
    return label_table(label_values, up.shape[0], up.device)[up.argmax(0)], margin_of(up), up


def near_tie_share(margin, probabilities):
    return float((margin < TAU[probabilities]).float().mean())


def judge(device_labels, up, label_values, probabilities):
    """Apply the acceptance rule to the device's label volume against the referee's interpoland `up` (same device as the labels).
    -> dict of counts; `ok` is the verdict."""
    tau = TAU[probabilities]
    K = up.shape[0]
    table = label_table(label_values, K, up.device)
    dev = device_labels.to(torch.int64)
    assert dev.shape == up.shape[1:], (tuple(dev.shape), tuple(up.shape))
    top = up.max(0).values
    ref = table[up.argmax(0)]
    margin = margin_of(up)
    dev_cls = torch.full_like(dev, -1)
    for k in range(K):
        dev_cls[dev == table[k]] = k
    near = margin < tau
    dev_val = up.gather(0, dev_cls.clamp(min=0)[None])[0]
    wrong_clear = (~near) & (dev != ref)
    wrong_near = near & ((dev_cls < 0) | (top - dev_val > tau))
    res = {"voxels": dev.numel(), "near_tie_share": float(near.float().mean()), "differ_from_referee": int((dev != ref).sum()),
           "not_a_label": int((dev_cls < 0).sum()), "wrong_clear": int(wrong_clear.sum()), "wrong_near": int(wrong_near.sum())}
    res["ok"] = res["wrong_clear"] == 0 and res["wrong_near"] == 0 and res["not_a_label"] == 0
    return res


# ---- the coordinate rule written out, float64 values (checks the referee itself) -----------------------------------------------------

def axis_taps(out_size, in_size):
    """i0, i1, l0, l1 per output index, the coordinates in float32 exactly as the rule states them."""
    scale = np.float32(in_size) / np.float32(out_size)
    o = np.arange(out_size, dtype=np.float32)
    src = np.maximum(scale * (o + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def brute_force_upsample(x, shape):
    """x [K, D, H, W] (any float) -> float64 [K, d, h, w]: the eight-tap sum in float64."""
    x = np.asarray(x, np.float64)
    z0, z1, lz0, lz1 = axis_taps(shape[0], x.shape[1])
    y0, y1, ly0, ly1 = axis_taps(shape[1], x.shape[2])
    x0, x1, lx0, lx1 = axis_taps(shape[2], x.shape[3])
    out = np.zeros((x.shape[0],) + tuple(shape), np.float64)
    for zi, lz in ((z0, lz0), (z1, lz1)):
        for yi, ly in ((y0, ly0), (y1, ly1)):
            for xi, lx in ((x0, lx0), (x1, lx1)):
                w = lz[:, None, None] * ly[None, :, None] * lx[None, None, :]
                out += x[:, zi[:, None, None], yi[None, :, None], xi[None, None, :]] * w[None]
    return out
