"""Time micformer_amd.intensity.augment_intensity on the loader's output (128^3 x 2 channels, float16) next to an ATen composition of
the same chain on the same GPU; one JSON line per batch size.

    python tools/bench_intensity.py [--batches 1,8] [--min-seconds 0.5] [--size 128]

Three parameter sets, the same row for every (sample, channel):
  full       noise 0.05, sigma 0.8 (radius 3), brightness 0.9, contrast 1.15, inverted gamma 1.3 with retain_stats
  blur       sigma 0.8 alone
  pointwise  the full set without the blur
<set>_ms: device events around >= min-seconds of calls with a preallocated `out` after warm-up (the whole call: the workspace
allocation from torch's cache and the seven launches).  <set>_aten_ms: what a user composes today, in float32 on the float16 batch: torch.randn_like
for the noise, three F.pad(mode="reflect") + F.conv3d passes with a 1-D kernel for the blur (torch's "reflect" does not repeat the
edge voxel as scipy's does; the cost is the same), amin / amax / mean / std reductions and pointwise ops for the rest, a final cast.
<set>_ratio = aten / ours (above 1: the kernels are faster).  <set>_GBps: the bytes a single fused pass would move (read and write
the float16 batch once) over our time -- a rate of the whole call, not a kernel's share of peak.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

#            sigma noise bright contrast gamma mode retain 0
SETS = {
    "full": (0.8, 0.05, 0.9, 1.15, 1.3, 2.0, 1.0, 0.0),
    "blur": (0.8, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0),
    "pointwise": (0.0, 0.05, 0.9, 1.15, 1.3, 2.0, 1.0, 0.0),
}


def timed(fn, min_seconds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, ms = 0, 0.0
    while ms < min_seconds * 1e3:
        n = max(1, calls or 4)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms += e0.elapsed_time(e1)
        calls += n
    return ms / calls


def aten_chain(image, row):
    """The chain of include/micformer_intensity.h out of ATen ops, one row of parameters for the whole batch."""
    sigma, noise_std, brightness, contrast, gamma, mode, retain = row[:7]
    B, C = image.shape[:2]
    dims = (2, 3, 4)
    x = image.float()
    if noise_std > 0:
        x = x + noise_std * torch.randn_like(x)
    if sigma > 0:
        r = int(4 * sigma + 0.5)
        k = torch.arange(-r, r + 1, dtype=torch.float32, device=x.device)
        w = torch.exp(-0.5 * k * k / (sigma * sigma))
        w = w / w.sum()
        x = x.reshape(B * C, 1, *x.shape[2:])
        x = F.conv3d(F.pad(x, (r, r, 0, 0, 0, 0), mode="reflect"), w.view(1, 1, 1, 1, -1))
        x = F.conv3d(F.pad(x, (0, 0, r, r, 0, 0), mode="reflect"), w.view(1, 1, 1, -1, 1))
        x = F.conv3d(F.pad(x, (0, 0, 0, 0, r, r), mode="reflect"), w.view(1, 1, -1, 1, 1))
        x = x.reshape(B, C, *x.shape[2:])
    if brightness != 1:
        x = x * brightness
    if contrast != 1:
        mn, lo, hi = x.mean(dims, keepdim=True), x.amin(dims, keepdim=True), x.amax(dims, keepdim=True)
        x = torch.minimum(torch.maximum((x - mn) * contrast + mn, lo), hi)
    if mode:
        if mode == 2:
            x = -x
        if retain:
            s0, m0 = torch.std_mean(x, dims, correction=0, keepdim=True)
        lo = x.amin(dims, keepdim=True)
        rng = x.amax(dims, keepdim=True) - lo
        x = torch.pow((x - lo) / (rng + 1e-7), gamma) * rng + lo
        if retain:
            s1, m1 = torch.std_mean(x, dims, correction=0, keepdim=True)
            x = (x - m1) / (s1 + 1e-8) * s0 + m0
        if mode == 2:
            x = -x
    return x.to(image.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--size", type=int, default=128)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_intensity.py needs the GPU")
    from micformer_amd.intensity import augment_intensity
    size = (a.size,) * 3
    for B in [int(b) for b in a.batches.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(B)
        image = torch.rand((B, 2) + size, generator=g, device="cuda").to(torch.float16)
        seeds = torch.arange(B, dtype=torch.int64, device="cuda")
        out = torch.empty_like(image)
        row = {"case": f"{B}x2x" + "x".join(map(str, size)) + " float16", "B": B}
        for name, values in SETS.items():
            params = torch.tensor(values, dtype=torch.float32).expand(B, 2, 8).contiguous().cuda()
            ours = timed(lambda: augment_intensity(image, params, seeds, out=out), a.min_seconds)
            aten = timed(lambda: aten_chain(image, values), a.min_seconds)
            got, ref = out.float(), aten_chain(image, values).float()
            row.update({f"{name}_ms": round(ours, 4), f"{name}_aten_ms": round(aten, 4), f"{name}_ratio": round(aten / ours, 2),
                        f"{name}_GBps": round(2 * image.numel() * 2 / ours / 1e6, 1)})
            if name == "blur":                                        # same data, same weights: away from the faces the two agree
                inner = (slice(None), slice(None)) + (slice(8, -8),) * 3
                row["blur_max_diff_vs_aten_inner"] = round(float((got[inner] - ref[inner]).abs().max()), 6)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
