"""Time micformer_amd.metrics.hausdorff_distance (HD95, include_background=False) on realistic label pairs; one JSON line per case.

    python tools/bench_metrics.py [--cases 128,512] [--min-seconds 0.5]

Pairs: gt = oracle.fill.make_label_map (nested shells split by angle), pred = gt shifted by (2, -1, 1) voxels with an
ellipsoid of class 3 pasted in.  ms_per_call: device events around >= min-seconds of calls after warm-up.  cpu_s: one CPU
restatement (scipy binary_erosion + distance_transform_edt per class, cropped to the class box) when scipy imports, else null.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = {"128": (1, 128, 128, 128), "512": (1, 512, 512, 256)}


def make_pair(B, D, H, W):
    from oracle import fill
    gt = fill.make_label_map(B, D, H, W)
    pred = torch.roll(gt, shifts=(2, -1, 1), dims=(1, 2, 3))
    z = torch.arange(D).view(1, D, 1, 1).float()
    y = torch.arange(H).view(1, 1, H, 1).float()
    x = torch.arange(W).view(1, 1, 1, W).float()
    ell = ((z - 0.55 * D) / (0.12 * D)) ** 2 + ((y - 0.45 * H) / (0.2 * H)) ** 2 + ((x - 0.5 * W) / (0.15 * W)) ** 2 <= 1
    pred = torch.where(ell.expand_as(pred), torch.full_like(pred, 3), pred)
    return pred.to(torch.uint8), gt.to(torch.uint8)


def cpu_seconds(pred, gt, K=8, percentile=95):
    try:
        from scipy import ndimage as nd
    except ImportError:
        return None
    p, g = pred[0].numpy(), gt[0].numpy()
    t0 = time.perf_counter()
    for c in range(1, K):
        pc, gc = p == c, g == c
        u = pc | gc
        if not u.any():
            continue
        idx = np.nonzero(u)
        box = tuple(slice(int(i.min()), int(i.max()) + 1) for i in idx)
        pc, gc = np.squeeze(pc[box]), np.squeeze(gc[box])
        ep, eg = nd.binary_erosion(pc) ^ pc, nd.binary_erosion(gc) ^ gc
        if ep.any() and eg.any():
            np.percentile(nd.distance_transform_edt(~eg)[ep], percentile)
            np.percentile(nd.distance_transform_edt(~ep)[eg], percentile)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="128,512")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py needs the GPU")
    from micformer_amd import metrics
    for name in a.cases.split(","):
        B, D, H, W = CASES[name]
        pred, gt = make_pair(B, D, H, W)
        p, g = pred.cuda(), gt.cuda()
        for _ in range(3):
            metrics.hausdorff_distance(p, g, num_classes=8, percentile=95)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        calls, ms = 0, 0.0
        while ms < a.min_seconds * 1e3:
            n = max(1, calls or 4)
            e0.record()
            for _ in range(n):
                out = metrics.hausdorff_distance(p, g, num_classes=8, percentile=95)
            e1.record()
            e1.synchronize()
            ms += e0.elapsed_time(e1)
            calls += n
        ws = int(metrics.lib.micf_surface_metrics_workspace(B, 8, D, H, W))
        cpu = None if a.no_cpu else cpu_seconds(pred, gt)
        print(json.dumps({"case": f"{D}x{H}x{W}", "B": B, "K": 8, "percentile": 95, "ms_per_call": round(ms / calls, 4),
                          "calls": calls, "workspace_bytes": ws, "cpu_s": None if cpu is None else round(cpu, 3),
                          "hd95": [round(float(v), 4) for v in out[0].cpu()]}), flush=True)


if __name__ == "__main__":
    main()
