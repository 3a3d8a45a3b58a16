"""Time micformer_amd.surface.surface_distances (HD95 + ASD / ASSD + surface Dice, include_background=False); one JSON line per case.

    python tools/bench_surface.py [--cases 128,ct] [--replays 20] [--no-cpu]

Cases: "128" = 128^3 at unit spacing, "ct" = 363x512x512 at a CT-like spacing (slices 0.7 mm, 0.35 mm in plane); K = 8, B = 1,
the label pairs of tools/bench_metrics.py.  ms: the median over `replays` replays of one captured call after warm-up, each
between device events.  voxel_hd_ms: metrics.hausdorff_distance (the voxel-unit kernels) on the same input, timed the same way:
the difference is what the spacing, the two extra metric families and the selection cost.  cpu_s: scipy binary_erosion +
distance_transform_edt(sampling=spacing) per class on the host cores when scipy imports, else null.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_metrics import make_pair  # noqa: E402

K = 8
CASES = {"128": ((1, 128, 128, 128), (1.0, 1.0, 1.0)), "ct": ((1, 363, 512, 512), (0.7, 0.35, 0.35))}
TAU = [1.0] * (K - 1)


def cpu_seconds(pred, gt, spacing):
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
        box = tuple(slice(int(i.min()), int(i.max()) + 1) for i in np.nonzero(u))
        pc, gc = pc[box], gc[box]
        ep, eg = nd.binary_erosion(pc) ^ pc, nd.binary_erosion(gc) ^ gc
        if ep.any() and eg.any():
            d = [nd.distance_transform_edt(~eg, sampling=spacing)[ep], nd.distance_transform_edt(~ep, sampling=spacing)[eg]]
            np.percentile(d[0], 95), np.percentile(d[1], 95), np.concatenate(d).mean(), sum((x <= 1.0).sum() for x in d)
    return time.perf_counter() - t0


def median_replay_ms(fn, replays):
    """Median device time of `replays` replays of fn() captured once (3 eager warm-up calls on a side stream first)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    graph.replay()
    torch.cuda.synchronize()
    ms = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="128,ct")
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface.py needs the GPU")
    from micformer_amd import metrics, surface
    for name in a.cases.split(","):
        (B, D, H, W), spacing = CASES[name]
        pred, gt = make_pair(B, D, H, W)
        p, g = pred.cuda(), gt.cuda()
        ws = torch.empty(surface.workspace_bytes(p.shape, K), dtype=torch.uint8, device="cuda")
        ms, r = median_replay_ms(lambda: surface.surface_distances(p, g, num_classes=K, spacing=spacing, percentiles=(95,),
                                                                   thresholds=TAU, workspace=ws), a.replays)
        del ws
        voxel_ms, _ = median_replay_ms(lambda: metrics.hausdorff_distance(p, g, num_classes=K, percentile=95), a.replays)
        cpu = None if a.no_cpu else cpu_seconds(pred, gt, spacing)
        print(json.dumps({"case": f"{D}x{H}x{W}", "B": B, "K": K, "spacing": spacing, "ms": round(ms, 4),
                          "voxel_hd_ms": round(voxel_ms, 4), "replays": a.replays,
                          "workspace_bytes": surface.workspace_bytes(p.shape, K),
                          "cpu_s": None if cpu is None else round(cpu, 3),
                          "hd95": [round(float(v), 4) for v in r.hd[0, :, 0].cpu()],
                          "assd": [round(float(v), 4) for v in r.assd[0].cpu()],
                          "nsd": [round(float(v), 4) for v in r.nsd[0].cpu()]}), flush=True)


if __name__ == "__main__":
    main()
