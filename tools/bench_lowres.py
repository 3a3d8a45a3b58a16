"""Time micformer_amd.lowres.simulate_low_resolution on the loader's output (128^3 x 2 channels, float16) next to an ATen
composition of the same operation on the same GPU and to scipy on the host; one JSON line per batch size.

    python tools/bench_lowres.py [--batches 1,8] [--rounds 5] [--min-seconds 0.2] [--size 128] [--no-scipy]

Three target sets, every channel on:
  half      zoom 0.5 on every axis (64^3)
  three_q   zoom 0.75 (96^3)
  mixed     a zoom per channel drawn from (0.5, 1) by draw_low_resolution(p_per_sample=1, p_per_channel=1)
<set>_ms: device events around >= min-seconds of calls with a preallocated `out` after warm-up (the whole call: the workspace
allocation from torch's cache and the four launches); the two candidates alternate over `rounds` rounds and the best round of each
counts.  <set>_aten_ms: what a user composes today, in float32 on the float16 batch: per axis the nearest gather and the dense
n x t matrix (interpolation . prefilter) are built on the host outside the timing; half and three_q run three index_select and three
einsum per call, mixed folds the gather into per-channel n x n matrices (zero columns beyond t) and runs three batched einsum.
<set>_ratio = aten / ours (above 1: the kernels are faster).  <set>_GBps: the bytes the call must move -- read `in`, write `out`,
write and read the float32 coefficients once -- over our time: a rate of the whole call, not a kernel's share of peak.
scipy_channel_ms: scipy.ndimage.zoom order 0 down and order 3 up of ONE 128^3 channel at zoom 0.5 on the host, once.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))                     # the float64 referee builds the matrices

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, min_seconds):
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


def alternate(fns, rounds, min_seconds):
    """-> the best round's ms per call of every candidate; the candidates take turns within a round."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    best = [float("inf")] * len(fns)
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            best[i] = min(best[i], timed(fn, min_seconds))
    return best


def axis_matrix(n, t):
    """[n, t] float64: output = matrix @ low along one axis (four B-spline taps of the prefiltered, edge-extended line)."""
    import lowres_ref as R
    coef = R.prefilter(np.eye(t), 0)                                  # [t + 4, t]: the prefilter is linear in the line
    fl, f = R.taps(n, t)
    m = np.zeros((n, t))
    for j, w in enumerate(R.bspline_weights(f)):
        m += w[:, None] * coef[fl - 1 + j + R.EXT]
    return m


def aten_uniform(image, t):
    import lowres_ref as R
    n = image.shape[2:]
    idx = [torch.from_numpy(R.gather_index(n[a], t[a])).cuda() for a in range(3)]
    mats = [torch.from_numpy(axis_matrix(n[a], t[a])).float().cuda() for a in range(3)]

    def run():
        x = image.float()
        x = x.index_select(2, idx[0]).index_select(3, idx[1]).index_select(4, idx[2])
        x = torch.einsum("bcdhw,Ww->bcdhW", x, mats[2])
        x = torch.einsum("bcdhw,Hh->bcdHw", x, mats[1])
        x = torch.einsum("bcdhw,Dd->bcDhw", x, mats[0])
        return x.to(image.dtype)
    return run


def aten_mixed(image, target):
    import lowres_ref as R
    B, C = image.shape[:2]
    n = image.shape[2:]
    mats = []
    for a in range(3):
        m = np.zeros((B, C, n[a], n[a]))
        for b in range(B):
            for c in range(C):
                t = int(target[b, c, a])
                m[b, c][:, R.gather_index(n[a], t)] += axis_matrix(n[a], t)     # the gather folded in: a column per source voxel
        mats.append(torch.from_numpy(m).float().cuda())

    def run():
        x = image.float()
        x = torch.einsum("bcdhw,bcWw->bcdhW", x, mats[2])
        x = torch.einsum("bcdhw,bcHh->bcdHw", x, mats[1])
        x = torch.einsum("bcdhw,bcDd->bcDhw", x, mats[0])
        return x.to(image.dtype)
    return run


def must_move(image, target):
    """bytes: read `in`, write `out`, write and read the coefficients [td + 4][th + 4][tw + 4] float32 of every channel"""
    coef = int((np.asarray(target, np.int64) + 4).prod(axis=2).sum()) * 4
    return 2 * image.numel() * image.element_size() + 2 * coef


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lowres.py needs the GPU")
    from micformer_amd.lowres import draw_low_resolution, simulate_low_resolution
    size = (a.size,) * 3
    scipy_ms = None
    if not a.no_scipy:
        from scipy import ndimage
        ch = np.random.default_rng(0).random(size).astype(np.float32)
        t0 = time.perf_counter()
        low = ndimage.zoom(ch, 0.5, order=0, mode="nearest", grid_mode=True)
        ndimage.zoom(low, [n / s for n, s in zip(size, low.shape)], order=3, mode="nearest", grid_mode=True)
        scipy_ms = (time.perf_counter() - t0) * 1e3
    for B in [int(b) for b in a.batches.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(B)
        image = torch.rand((B, 2) + size, generator=g, device="cuda").to(torch.float16)
        out = torch.empty_like(image)
        mixed = draw_low_resolution(B, size, generator=torch.Generator().manual_seed(B), p_per_sample=1.0, p_per_channel=1.0)
        sets = {"half": torch.tensor([s // 2 for s in size], dtype=torch.int32).expand(B, 2, 3).contiguous(),
                "three_q": torch.tensor([3 * s // 4 for s in size], dtype=torch.int32).expand(B, 2, 3).contiguous(),
                "mixed": mixed}
        row = {"case": f"{B}x2x" + "x".join(map(str, size)) + " float16", "B": B}
        for name, target in sets.items():
            td = target.cuda()
            aten = aten_mixed(image, target.numpy()) if name == "mixed" else aten_uniform(image, target[0, 0].tolist())
            ours_ms, aten_ms = alternate([lambda: simulate_low_resolution(image, td, out=out), aten], a.rounds, a.min_seconds)
            nbytes = must_move(image, target.numpy())
            row.update({f"{name}_ms": round(ours_ms, 4), f"{name}_aten_ms": round(aten_ms, 4), f"{name}_ratio": round(aten_ms / ours_ms, 2),
                        f"{name}_GBps": round(nbytes / ours_ms / 1e6, 1),
                        f"{name}_max_diff_vs_aten": round(float((out.float() - aten().float()).abs().max()), 6)})
        if scipy_ms is not None:
            row["scipy_channel_ms"] = round(scipy_ms, 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
