"""Time micformer_amd.loader.load_batch on a full-size MM-WHS-like pair (363x512x512 int16 CT + float32 MR + int16 CT label -> 128^3);
one JSON line per batch size.

    python tools/bench_loader.py [--batches 1,4] [--min-seconds 0.5] [--no-cpu] [--normalisation minmax|zscore|percentile|CT,MR]
                                 [--affine [--padding-mode zeros|border]]
                                 [--elastic [--field-grid N] [--field-interpolation linear|cubic]]

ms_per_call: device events around >= min-seconds of calls after warm-up (the whole call: workspace zeroing, min/max, resize + label + crop,
crop finish).  minmax_ms: the same call with a 1x1x1 target, i.e. the full read of the raw image volumes plus launch overheads;
minmax_GBps: the raw image bytes of the batch (the bytes that pass must read) over that time.  resize_ms: the difference of the two.
Per-kernel times proper come from a kernel trace of this script (loader_zero_kernel / loader_minmax_kernel /
resize_kernel<LoaderWords> / loader_crop_kernel; with --normalisation norm_minmax_kernel, norm_moments_kernel, norm_hist_kernel,
norm_scan_kernel, norm_finish_kernel and resize_kernel<NormWords>; with --affine affine_resample_kernel).
cpu_s: the CPU referee (tests/loader_ref.py: numpy + F.interpolate, the reference's own operators) for ONE sample on this host.
--normalisation other than the default "minmax" times the same call through micf_volume_loader_norm (csrc/volume_normalise.hip):
the 1x1x1-target call is then the statistics passes of that mode (moments; histogram + scan per digit), reported as stats_ms /
stats_GBps against the same raw image bytes read ONCE (the percentile mode reads them two or three times), and cpu_s is
tests/normalise_ref.py.
--affine times the same call with a drawn map per sample (affine.draw_affine, csrc/volume_affine.hip) next to the call without one:
affine_ms_per_call against plain_ms_per_call, affine_stats_ms (the 1x1x1-target call: the statistics passes, which do not depend on
the map) and affine_resample_ms (the difference), plus grid_sample_ms: F.affine_grid + F.grid_sample (bilinear) on the already
loaded float16 image of the batch with the same maps, the second resample a user would run today (the label would need a third).
There is no bar; the raw-volume statistics pass should still dominate.
--elastic times the same call with a drawn displacement field per sample (elastic.draw_elastic on an N^3 control grid, default 7,
csrc/volume_elastic.hip: elastic_resample_kernel), composed with the drawn map when --affine is given too: elastic_ms_per_call next
to the affine and plain calls, elastic_stats_ms / elastic_resample_ms as above, and dense_grid_sample_ms: F.grid_sample (bilinear)
of the already loaded float16 image on a dense [B, 128, 128, 128, 3] grid (F.affine_grid of the maps, or of the identity, plus the
field upsampled to one vector per voxel once, outside the timing), the second resample this replaces.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPE = (363, 512, 512)
SIZE = (128, 128, 128)


def make_sample(seed):
    import loader_ref
    g = np.random.default_rng(seed)
    ct = g.integers(-1024, 3072, size=SHAPE, dtype=np.int16)
    mr = g.random(SHAPE, dtype=np.float32) * np.float32(1200.0)
    values = np.array((0,) + loader_ref.MMWHS_LABEL_VALUES, np.int16)
    lab = values[g.integers(0, len(values), size=SHAPE)]
    return ct, mr, lab


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
    return ms / calls, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--normalisation", default="minmax", help="one mode for both channels, or CT,MR")
    ap.add_argument("--affine", action="store_true", help="also time the call with a drawn affine map per sample")
    ap.add_argument("--padding-mode", default="zeros", choices=["zeros", "border"])
    ap.add_argument("--elastic", action="store_true", help="also time the call with a drawn displacement field per sample")
    ap.add_argument("--field-grid", type=int, default=7, help="control points per axis of the drawn field")
    ap.add_argument("--field-interpolation", default="cubic", choices=["linear", "cubic"])
    a = ap.parse_args()
    norm = tuple(a.normalisation.split(",")) if "," in a.normalisation else a.normalisation
    default = norm == "minmax"
    if not torch.cuda.is_available():
        raise SystemExit("bench_loader.py needs the GPU")
    import loader_ref
    from micformer_amd import loader
    batches = [int(b) for b in a.batches.split(",")]
    host = make_sample(0)
    cpu = None
    if not a.no_cpu:
        t0 = time.perf_counter()
        if default:
            loader_ref.load_pair(*host, size=SIZE)
        else:
            import normalise_ref
            normalise_ref.load_pair(*host, size=SIZE, normalisation=norm)
        cpu = time.perf_counter() - t0
    first = tuple(torch.from_numpy(x).cuda() for x in host)
    samples = [first] + [tuple(t.clone() for t in first) for _ in range(max(batches) - 1)]      # distinct buffers per sample
    raw_bytes = sum(t.numel() * t.element_size() for t in first[:2])
    for B in batches:
        dev = samples[:B]
        out = (torch.empty((B, 2) + SIZE, dtype=torch.float16, device="cuda"),
               torch.empty((B,) + SIZE, dtype=torch.uint8, device="cuda"), torch.empty((B, 3, 2), dtype=torch.int32, device="cuda"))
        tiny = (torch.empty((B, 2, 1, 1, 1), dtype=torch.float16, device="cuda"),
                torch.empty((B, 1, 1, 1), dtype=torch.uint8, device="cuda"), torch.empty((B, 3, 2), dtype=torch.int32, device="cuda"))
        kw = {} if default else {"normalisation": norm}
        total, calls = timed(lambda: loader.load_batch(dev, size=SIZE, out=out, **kw), a.min_seconds)
        mm, _ = timed(lambda: loader.load_batch(dev, size=(1, 1, 1), out=tiny, **kw), a.min_seconds)
        first_pass = "minmax" if default else "stats"
        row = {"case": "x".join(map(str, SHAPE)) + " -> " + "x".join(map(str, SIZE)), "B": B,
               "ms_per_call": round(total, 4), "ms_per_pair": round(total / B, 4), "calls": calls,
               first_pass + "_ms": round(mm, 4), first_pass + "_GBps": round(B * raw_bytes / mm / 1e6, 1),
               "resize_ms": round(total - mm, 4), "raw_image_bytes_per_pair": raw_bytes,
               "cpu_s": None if cpu is None else round(cpu, 3),
               "crop_indexes": out[2][0].cpu().tolist()}
        if not default:
            row["normalisation"] = a.normalisation
        if a.affine:
            import torch.nn.functional as F
            from micformer_amd import affine
            theta = affine.draw_affine(B, size=SIZE, generator=torch.Generator().manual_seed(B), device="cuda")
            akw = dict(kw, affine=theta, padding_mode=a.padding_mode)
            at, _ = timed(lambda: loader.load_batch(dev, size=SIZE, out=out, **akw), a.min_seconds)
            ast, _ = timed(lambda: loader.load_batch(dev, size=(1, 1, 1), out=tiny, **akw), a.min_seconds)
            image = out[0].clone()
            gs, _ = timed(lambda: F.grid_sample(image, F.affine_grid(theta, image.shape, align_corners=False).to(image.dtype),
                                                mode="bilinear", padding_mode=a.padding_mode, align_corners=False), a.min_seconds)
            row.update({"padding_mode": a.padding_mode, "plain_ms_per_call": row["ms_per_call"], "affine_ms_per_call": round(at, 4),
                        "affine_stats_ms": round(ast, 4), "affine_resample_ms": round(at - ast, 4),
                        "affine_minus_plain_ms": round(at - total, 4), "grid_sample_ms": round(gs, 4)})
        if a.elastic:
            import torch.nn.functional as F
            from micformer_amd import affine, elastic
            grid = (a.field_grid,) * 3
            spacing = (SIZE[0] - 1) / (a.field_grid - 1)
            field = elastic.draw_elastic(B, size=SIZE, grid=grid, magnitude=min(5.0, 0.4 * spacing),
                                         generator=torch.Generator().manual_seed(100 + B), device="cuda")
            theta = affine.draw_affine(B, size=SIZE, generator=torch.Generator().manual_seed(B), device="cuda") if a.affine else None
            ekw = dict(kw, displacement=field, field_interpolation=a.field_interpolation, affine=theta, padding_mode=a.padding_mode)
            et, _ = timed(lambda: loader.load_batch(dev, size=SIZE, out=out, **ekw), a.min_seconds)
            est, _ = timed(lambda: loader.load_batch(dev, size=(1, 1, 1), out=tiny, **ekw), a.min_seconds)
            image = out[0].clone()
            eye = torch.eye(3, 4, device="cuda").expand(B, 3, 4)
            dense = F.interpolate(field, size=SIZE, mode="trilinear", align_corners=True).permute(0, 2, 3, 4, 1)
            dense = (F.affine_grid(eye if theta is None else theta, image.shape, align_corners=False) + dense).to(image.dtype)
            gs, _ = timed(lambda: F.grid_sample(image, dense, mode="bilinear", padding_mode=a.padding_mode, align_corners=False),
                          a.min_seconds)
            row.update({"padding_mode": a.padding_mode, "field_grid": list(grid), "field_interpolation": a.field_interpolation,
                        "plain_ms_per_call": row["ms_per_call"], "elastic_ms_per_call": round(et, 4),
                        "elastic_stats_ms": round(est, 4), "elastic_resample_ms": round(et - est, 4),
                        "elastic_minus_plain_ms": round(et - total, 4), "dense_grid_sample_ms": round(gs, 4)})
            if a.affine:
                row["elastic_minus_affine_ms"] = round(et - row["affine_ms_per_call"], 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
